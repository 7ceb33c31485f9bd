"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the reference's fixtures.

Tolerances (fp32): Potts energies |d| <= 5e-6 * max(1, |e|) (+ 5e-6 * lamda for the fitness term of
a product of experts), fitness 5e-6, gradients 2e-6 * max(1, lamda); sampled indices, accept bits, best states:
exact. The largest observed error / tolerance ratios are appended to gpurun_out/parity_observed.json.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppde_oracle as orc
from helpers import GOLDEN, fixture_noise, load, model_from_fixture, oracle_energy
from ppde_amd import synthetic
from ppde_amd.encoding import seqs_to_idx


def hip_model(J, h, i0, wt_idx, cnn, lamda):
    from ppde_amd.energy import HipModel
    m = HipModel(wt_idx, "cuda:0")
    m.set_potts(J, h, i0)
    if cnn is not None:
        m.set_cnn(cnn)
    m.set_lamda(lamda)
    return m


def e_tol(e, lam=0.0):
    return 5e-6 * np.maximum(1.0, np.abs(e)) + 5e-6 * lam


def observed(tag, err, tol):
    """Record max(err / tol) of a check next to the test run (gpurun_out/ travels back from the GPU box)."""
    import json
    ratio = float(np.max(np.asarray(err, dtype=np.float64) / np.asarray(tol, dtype=np.float64)))
    path = os.path.join(os.path.dirname(GOLDEN), "..", "gpurun_out", "parity_observed.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        d = json.load(open(path)) if os.path.exists(path) else {}
        d[tag] = {"max_err_over_tol": ratio, "max_abs_err": float(np.max(err))}
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    print(f"[parity] {tag}: max |err| {float(np.max(err)):.3e} = {ratio:.2f} of the tolerance")
    return ratio


@pytest.mark.parametrize("name", ["ops_toy24_lam5.npz", "ops_pabp_lam5.npz", "ops_pabp_lam0.npz", "ops_toy24_nonsym.npz"])
def test_energy_grad_vs_reference_fixture(name):
    fx = load(name)
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    lam = float(fx["lamda"])
    m = hip_model(J, h, i0, wt_idx, cnn, lam)
    idx = torch.as_tensor(fx["idx"]).cuda()
    wt_H = float(np.ravel(fx["wt_H"])[0])
    assert abs(m.wt_hamiltonian - wt_H) <= 4e-6 * (abs(wt_H) + 1)
    e, fit, g = m.energy_grad(idx, 3)
    assert observed(f"{name}:e", np.abs(e.cpu().numpy() - fx["e"]), e_tol(fx["e"], lam)) <= 1.0
    assert np.abs(fit.cpu().numpy() - fx["fit"]).max() <= 5e-6
    assert np.abs(g.cpu().numpy() - fx["grad"]).max() <= 2e-6 * max(1.0, lam)
    e1, f1, g1 = m.energy_grad(idx, 1)
    assert observed(f"{name}:potts_e", np.abs(e1.cpu().numpy() - fx["unsupervised"]), e_tol(fx["unsupervised"])) <= 1.0
    assert float(f1.abs().max()) == 0.0
    e2, f2, g2 = m.energy_grad(idx, 2)
    assert np.abs(f2.cpu().numpy() - fx["supervised"]).max() <= 5e-6
    assert np.abs(e2.cpu().numpy() - fx["supervised"]).max() <= 5e-6
    assert np.abs(g2.cpu().numpy() - fx["supervised_grad"]).max() <= 2e-6
    # the wild type's Delta-H is exactly zero, as in the reference
    e_wt, _, _ = m.energy_grad(torch.as_tensor(wt_idx).reshape(1, -1).cuda(), 1)
    assert float(e_wt[0]) == 0.0


def _check_trained(tag, fx, out, label, prefix=""):
    """HIP outputs on the trained networks (dict f2 / e2 / g2 / e / fit / g) against what the REFERENCE computed from the
    same checkpoint files (real_<tag>.npz): SURVEY 8(c)'s tolerances, relative for values beyond 1."""
    lam = float(fx["lamda"])
    ftol = 4e-6 * np.maximum(1.0, np.abs(fx["supervised"]))
    assert observed(f"{prefix}real_{tag}{label}:supervised", np.abs(out["f2"] - fx["supervised"]), ftol) <= 1.0
    assert np.array_equal(out["e2"], out["f2"])
    gs = max(1.0, float(np.abs(fx["supervised_grad"]).max()))
    assert observed(f"{prefix}real_{tag}{label}:supervised_grad", np.abs(out["g2"] - fx["supervised_grad"]).max(), 2e-6 * gs) <= 1.0
    assert observed(f"{prefix}real_{tag}{label}:fit", np.abs(out["fit"] - fx["fit"]), ftol) <= 1.0
    assert observed(f"{prefix}real_{tag}{label}:e", np.abs(out["e"] - fx["e"]), e_tol(fx["e"], lam) + 4e-6 * lam * np.maximum(1.0, np.abs(fx["fit"]))) <= 1.0
    assert observed(f"{prefix}real_{tag}{label}:grad", np.abs(out["g"] - fx["grad"]).max(), 2e-6 * max(1.0, lam) * max(1.0, float(np.abs(fx["grad"]).max()))) <= 1.0


@pytest.mark.parametrize("tag", ["pabp", "ube4b", "gfp"])
def test_trained_cnn_weights_through_the_hip_kernels(tag):
    """The HIP CNN kernels on the TRAINED weights of all three proteins (tests/golden/real_<tag>_cnn.npz, the shipped
    checkpoints' values) against the outputs the REFERENCE computed from those files (real_<tag>.npz): which = 2
    (ProteinSupervised) and which = 3 (Potts product of experts, lamda as the README recommends, synthetic couplings). PABP
    takes the single-launch kernel, UBE4B (L = 104) and GFP (L = 237) the chunked forward / backward pair -- the supervised
    expert of BASELINE configs 5 and 4. Trained networks have saturated / dead features and exact ties at the max over
    positions that seeded-uniform weights never show."""
    from helpers import real_cnn_states
    fx = load(f"real_{tag}.npz")
    cnn, _ = real_cnn_states(tag)
    J, h = synthetic.make_potts(int(fx["Lp"]), seed=int(fx["potts_seed"]))
    lam = float(fx["lamda"])
    m = hip_model(J, h, int(fx["win_start"]), fx["wt_idx"], cnn, lam)
    idx = torch.as_tensor(fx["idx"]).cuda()
    e2, f2, g2 = m.energy_grad(idx, 2)
    e, fit, g = m.energy_grad(idx, 3)
    c = lambda t: t.cpu().numpy()
    _check_trained(tag, fx, dict(e2=c(e2), f2=c(f2), g2=c(g2), e=c(e), fit=c(fit), g=c(g)), "")
    # and a short sampler run on them against the oracle (device RNG, oracle fed the device's noise)
    from helpers import device_noise
    from ppde_amd.sampler import Chains
    n, T, pas, i0, Lp = 16, 25, 2, int(fx["win_start"]), int(fx["Lp"])
    wt = fx["wt_idx"]
    ch = Chains(m, n, T, pas, 6, False, i0, i0 + Lp - 1, 3, 1, trace=True, random_chain=0, seed=31, use_graph=False)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    ref = orc.run(oracle_energy(J, h, i0, wt, cnn, lam), np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, i0, i0 + Lp - 1,
                  pas, 6, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert observed(f"real_{tag}:run_energy_history", np.abs(res["energy_history"] - ref["energy_history"].numpy()),
                    e_tol(ref["energy_history"].numpy(), lam) + 4e-6 * lam * np.maximum(1.0, np.abs(ref["fitness_history"].numpy()))) <= 1.0


_TRAINED_KNOBS = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from helpers import load, real_cnn_states
from ppde_amd import synthetic
from test_hip_parity import hip_model
out = {}
for tag in ("pabp", "ube4b", "gfp"):
    fx = load(f"real_{tag}.npz")
    cnn, _ = real_cnn_states(tag)
    J, h = synthetic.make_potts(int(fx["Lp"]), seed=int(fx["potts_seed"]))
    m = hip_model(J, h, int(fx["win_start"]), fx["wt_idx"], cnn, float(fx["lamda"]))
    idx = torch.as_tensor(fx["idx"]).cuda()
    for k, v in zip(("e2", "f2", "g2"), m.energy_grad(idx, 2)): out[f"{tag}.{k}"] = v.cpu().numpy()
    for k, v in zip(("e", "fit", "g"), m.energy_grad(idx, 3)): out[f"{tag}.{k}"] = v.cpu().numpy()
    m.close()
np.savez(sys.argv[2], **out)
"""


def test_trained_cnn_weights_under_every_kernel_form():
    """The trained networks of the three proteins through every form the supervised expert's kernels exist in: the
    split-precision bf16 contractions (default) and the exact-fp32 MFMA ones (PPDE_CNN_BF16=0), each with the long proteins'
    chunk kernels at 512 (default above 128 channels) or 256 threads, and the general instead of the shape-pinned
    instantiations. Every form within SURVEY's tolerances of the REFERENCE's outputs; forms that only differ in the launch
    geometry are bit-identical."""
    import subprocess
    import sys
    import tempfile
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    forms = (("bf16", {}), ("bf16_256", {"PPDE_CNN_CHUNK_512": "0"}), ("bf16_general", {"PPDE_CNN_SPEC": "0"}),
             ("fp32", {"PPDE_CNN_BF16": "0"}), ("fp32_256", {"PPDE_CNN_BF16": "0", "PPDE_CNN_CHUNK_512": "0"}))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "trained_knobs.py")
        open(script, "w").write(_TRAINED_KNOBS)
        for name, env in forms:
            out = os.path.join(d, name + ".npz")
            r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=400, env=dict(os.environ, **env))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            res[name] = dict(np.load(out))
    for tag in ("pabp", "ube4b", "gfp"):
        fx = load(f"real_{tag}.npz")
        for name, _ in forms:
            _check_trained(tag, fx, {k.split(".", 1)[1]: v for k, v in res[name].items() if k.startswith(tag + ".")}, ":" + name)
    for a_, b_ in (("bf16", "bf16_256"), ("bf16", "bf16_general"), ("fp32", "fp32_256")):
        for k in res[a_]:
            assert np.array_equal(res[a_][k], res[b_][k]), (a_, b_, k)


@pytest.mark.parametrize("n", [1, 3, 64, 65, 128, 200, 600])
def test_energy_grad_vs_oracle_batch_sizes(n):
    """Ragged batch sizes through every chain-group instantiation; also checks batch-independence bit for bit."""
    fx = load("ops_pabp_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = hip_model(J, h, i0, wt_idx, cnn, 5.0)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 20, size=(n, wt_idx.shape[0])).astype(np.uint8)
    e, fit, g = m.energy_grad(torch.as_tensor(idx).cuda(), 3)
    en = oracle_energy(J, h, i0, wt_idx, cnn, 5.0)
    eo, fo, go = en.energy_grad(torch.as_tensor(idx.astype(np.int64)))
    wt_H = float(en.potts.wt_H)
    assert observed(f"batch{n}:e_vs_oracle", np.abs(e.cpu().numpy() - eo.numpy()), e_tol(eo.numpy(), 5.0)) <= 1.0
    assert np.abs(fit.cpu().numpy() - fo.numpy()).max() <= 5e-6
    # the max over t picks a row: a chain's routed gradient may differ from the oracle's only where the fp64 evaluation shows two
    # rows tied to within matmul rounding, or a pre-activation at the ReLU kink (numerics contract) -- and then it must
    # be the gradient of another admissible routing, within the same tolerance (helpers.classify_chain_gradient)
    from helpers import vet_gradient_outliers
    _, gc = en.cnn.fit_grad(torch.as_tensor(idx.astype(np.int64)))
    dg, unresolved = vet_gradient_outliers(g.cpu().numpy(), go.numpy(), gc.numpy(), cnn, idx, 1e-5, lamda=5.0, label=f"batch{n}")
    assert dg[np.setdiff1d(np.arange(n), unresolved)].max() <= 1e-5
    # a chain's numbers do not depend on which batch it sits in
    e1, f1, g1 = m.energy_grad(torch.as_tensor(idx[:1]).cuda(), 3)
    assert torch.equal(e1, e[:1]) and torch.equal(f1, fit[:1]) and torch.equal(g1, g[:1])


def test_not_onehot_is_rejected():
    fx = load("ops_toy24_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = hip_model(J, h, i0, wt_idx, cnn, 5.0)
    x = m.idx_to_onehot(torch.as_tensor(fx["idx"]).cuda())
    assert torch.equal(m.onehot_to_idx(x).cpu(), torch.as_tensor(fx["idx"]))
    x[0, 3] = 0.25
    with pytest.raises(ValueError):
        m.onehot_to_idx(x)


def _chains(m, fx, n, T, rng_mode, **kw):
    from ppde_amd.sampler import Chains
    return Chains(m, n, T, int(fx["pas"]), int(fx["nmut"]), bool(fx["paper"]), int(fx["min_pos"]), int(fx["max_pos"]),
                  3, rng_mode, trace=True, random_chain=int(fx["random_idx"]), **kw)


def _feed(ch, noise, n, lo=0, hi=None):
    for U, q, u in noise:
        hi_ = hi if hi is not None else n
        ch.run(1, (U[lo:hi_].to(torch.int32).reshape(1, -1), q[:, lo:hi_].contiguous(), u[lo:hi_].reshape(1, -1), [int(q.shape[0])]))


RUNS_Q = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "run_toy24_*.npz")))
RUNS_ALL = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "run_*.npz")))


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("name", RUNS_Q)
def test_sampler_replays_reference_trajectory(name, reuse):
    """HIP path vs the REFERENCE's own recorded run (noise stored in the fixture)."""
    fx = load(name)
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    lam, n, T, pas = float(fx["lamda"]), int(fx["n"]), int(fx["T"]), int(fx["pas"])
    noise, _ = fixture_noise(fx, n, wt_idx.shape[0] * 20, pas, T)
    m = hip_model(J, h, i0, wt_idx, cnn, lam)
    ch = _chains(m, fx, n, T, 0, reuse_grad=reuse)
    ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    _feed(ch, noise, n)
    tr, res = ch.trace(), ch.collect()
    U = fx["U"]
    for t in range(T):
        for s in range(int(U[t].max())):
            act = s < U[t]
            assert np.array_equal(tr["flat"][t, s][act], fx["flat"][t, s][act]), f"draw differs at iteration {t} sub-step {s}"
    assert np.array_equal(tr["accepted"].astype(bool), fx["accepted"])
    assert np.abs(res["energy_history"] - fx["energy_history"]).max() <= 2e-5
    assert np.abs(res["fitness_history"] - fx["fitness_history"].reshape(T + 1, n)).max() <= 5e-6    # (the reference returns (T+1,) for one chain)
    assert np.array_equal(res["best_idx"], fx["best_idx"])
    assert np.abs(res["best_energy"] - fx["best_energy"]).max() <= 2e-5
    assert np.array_equal(res["random_traj"], fx["random_traj"])
    # the reference's --device cpu aliasing of recorded states
    ch2 = _chains(m, fx, n, T, 0, reuse_grad=reuse, record_after_reset=True)
    ch2.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    _feed(ch2, noise, n)
    res2 = ch2.collect()
    assert np.array_equal(res2["best_idx"], fx["best_idx_cpu_alias"])
    assert np.array_equal(res2["random_traj"], fx["random_traj_cpu_alias"])


@pytest.mark.parametrize("name", [r for r in RUNS_ALL if "pabp" in r])
def test_sampler_vs_oracle_pabp(name):
    """PABP-size runs: same locally drawn noise into the oracle and the HIP path."""
    fx = load(name)
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    lam, n, T, pas = float(fx["lamda"]), int(fx["n"]), int(fx["T"]), int(fx["pas"])
    L = wt_idx.shape[0]
    torch.manual_seed(int(fx["seed"]))
    noise = [orc.draw_noise_torch(n, L * 20, pas) for _ in range(T)]
    en = oracle_energy(J, h, i0, wt_idx, cnn, lam)
    kw = dict(num_steps=T, min_pos=int(fx["min_pos"]), max_pos=int(fx["max_pos"]), pas_length=pas,
              nmut_threshold=int(fx["nmut"]), paper_results=bool(fx["paper"]))
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], trace=True, **kw)
    m = hip_model(J, h, i0, wt_idx, cnn, lam)
    ch = _chains(m, fx, n, T, 0)
    ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    _feed(ch, noise, n)
    tr, res = ch.trace(), ch.collect()
    for t in range(T):
        U = noise[t][0].numpy()
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, int(fx["random_idx"])].numpy())


def _philox_setup(n=16, T=12, pas=2, nmut=3, lam=5.0):
    fx = load("ops_pabp_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = hip_model(J, h, i0, wt_idx, cnn, lam)
    return fx, J, h, i0, wt_idx, cnn, m


def test_philox_stream_matches_numpy():
    from ppde_amd.sampler import Chains
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    n, N = 8, wt_idx.shape[0] * 20
    seed, off = 0x1234567887654321, 40
    ch = Chains(m, n, 4, 2, 0, False, i0, i0 + J.shape[0] - 1, 1, 1, seed=seed, chain_offset=off)
    for it, s in [(0, 0), (3, 1), (7, 2)]:
        q, u, U = ch.philox_dump(it, s)
        k = np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint32)
        chain = (off + np.arange(n)).astype(np.uint32)
        qe = orc.device_race_variates(seed, off, n, it, s, N // 20)          # two-level draw: L residue + 20 letter variates
        assert q.shape == (n, N // 20 + 20)
        assert np.abs(q.cpu().numpy() - qe).max() <= 4e-7 * np.abs(qe).max() + 1e-12
        c1 = np.zeros((n, 4), dtype=np.uint32); c1[:, 0] = chain; c1[:, 1] = it; c1[:, 2] = 1
        ue = (orc.philox4x32(c1, k)[:, 0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)
        assert np.array_equal(u.cpu().numpy(), ue)
        c0 = np.zeros((n, 4), dtype=np.uint32); c0[:, 0] = chain; c0[:, 1] = it
        Ue = 1 + ((orc.philox4x32(c0, k)[:, 0].astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
        assert np.array_equal(U.cpu().numpy().astype(np.int64), Ue)


def _philox_run(m, n, T, pas, nmut, paper, i0, Lp, wt_idx, off=0, rows=None, which=3, trace=True, **kw):
    from ppde_amd.sampler import Chains
    lo, hi = rows if rows else (0, n)
    ch = Chains(m, hi - lo, T, pas, nmut, paper, i0, i0 + Lp - 1, which, 1, trace=trace, random_chain=0,
                seed=99, chain_offset=off + lo, **kw)
    ch.init(torch.as_tensor(np.tile(wt_idx, (hi - lo, 1))).cuda())
    ch.run(T)
    return ch, ch.trace() if trace else None, ch.collect()


def test_philox_mode_vs_oracle_and_invariances():
    """Device-RNG mode: (a) equals the oracle fed with the device's own noise; (b) identical bits with and without
    gradient reuse, with and without graph replay, on 1/3/4/8 HIP streams, and when the chains are split in two shards."""
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    n, T, pas, nmut = 16, 45, 2, 3
    Lp, L = J.shape[0], wt_idx.shape[0]
    ch, tr, res = _philox_run(m, n, T, pas, nmut, False, i0, Lp, wt_idx, use_graph=False)
    noise = []
    for t in range(T):
        qs = []
        for s in range(2 * pas - 1):
            q, u, U = ch.philox_dump(t, s)
            qs.append(q.cpu())
        noise.append((U.cpu().long(), torch.stack(qs, 0), u.cpu()))
    en = oracle_energy(J, h, i0, wt_idx, cnn, 5.0)
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, nmut, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    for kw in (dict(reuse_grad=False, use_graph=False), dict(use_graph=True), dict(reuse_grad=False, use_graph=True),
               dict(use_graph=False, n_streams=3), dict(use_graph=True, n_streams=4), dict(reuse_grad=False, use_graph=True, n_streams=8)):
        _, tr2, res2 = _philox_run(m, n, T, pas, nmut, False, i0, Lp, wt_idx, **kw)
        for k in ("energy_history", "fitness_history", "best_idx", "best_energy", "best_step"):
            assert np.array_equal(res[k], res2[k]), (kw, k)
        assert np.array_equal(tr["flat"], tr2["flat"]) and np.array_equal(tr["accepted"], tr2["accepted"])
    a = _philox_run(m, n, T, pas, nmut, False, i0, Lp, wt_idx, rows=(0, 7))[2]
    b = _philox_run(m, n, T, pas, nmut, False, i0, Lp, wt_idx, rows=(7, 16))[2]
    assert np.array_equal(np.concatenate([a["energy_history"], b["energy_history"]], 1), res["energy_history"])
    assert np.array_equal(np.concatenate([a["best_idx"], b["best_idx"]], 0), res["best_idx"])


@pytest.mark.parametrize("which,nmut,reuse", [(1, 0, False), (1, 0, True), (1, 3, False), (1, 3, True), (3, 0, False), (3, 0, True), (3, 4, True), (3, 4, False)])
def test_specialised_chain_kernels_equal_the_general_ones(which, nmut, reuse):
    """The chain kernels are instantiated once in general form and once per common configuration with that configuration's
    fields pinned to constants (pas.h pin_config: device RNG, no trace, experts, mutation cap or none, evaluation policy).
    A run WITHOUT trace buffers takes the specialised instantiation, the same run WITH them the general one (the one every
    oracle comparison above goes through): histories, best states and the recorded trajectory must be bit-identical."""
    from ppde_amd.sampler import Chains
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    n, T, Lp = 24, 130, J.shape[0]
    res = []
    for trace in (False, True):
        ch = Chains(m, n, T, 2, nmut, False, i0, i0 + Lp - 1, which, 1, reuse_grad=reuse, trace=trace, random_chain=5, seed=4242,
                    use_graph=True)
        ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
        ch.run(T)
        res.append(ch.collect())
    for k in ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert (res[0]["energy_history"][1:] != res[0]["energy_history"][:-1]).any()


@pytest.mark.parametrize("which", [1, 3])
def test_full_size_properties(which):
    """BASELINE config sizes (128 chains, PABP; which = 1: config 2's Potts product of experts, 3: config 3's Potts + CNN):
    properties that need no oracle run, and every way of issuing the same run gives the same bits."""
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    n, T, Lp, L = 128, 300, J.shape[0], wt_idx.shape[0]
    ch, tr, res = _philox_run(m, n, T, 2, 10, False, i0, Lp, wt_idx, which=which)
    eh = res["energy_history"]
    assert np.isfinite(eh).all()
    assert np.array_equal(res["best_energy"], eh.max(0))                        # running best == max over history
    assert np.array_equal(res["best_step"], eh.argmax(0))                       # first index on ties
    assert (res["best_idx"] < 20).all()
    # the recorded best state really has the recorded best energy
    e, f, _ = m.energy_grad(torch.as_tensor(res["best_idx"]).cuda(), which, want_grad=False)
    assert np.array_equal(e.cpu().numpy(), res["best_energy"])
    assert np.array_equal(f.cpu().numpy(), res["best_fitness"])
    # a rejected step repeats the previous energy exactly; an accepted one generally changes it
    acc = tr["accepted"].astype(bool)
    pk = ch.peek()
    assert (pk["dist"] < 10).all()                                              # mutation cap enforced after every step
    # a rejected step repeats the energy it started from: the previous row, or the wild type's after a cap reset
    e_wt = m.energy_grad(torch.as_tensor(wt_idx).reshape(1, -1).cuda(), which, want_grad=False)[0].cpu().numpy()[0]
    same = (eh[1:] == eh[:-1]) | (eh[1:] == e_wt)
    assert same[~acc].all()
    assert 0.02 < acc.mean() < 0.98
    # 100-iteration graph replays + the eager remainder == every iteration launched eagerly
    _, tr2, res2 = _philox_run(m, n, T, 2, 10, False, i0, Lp, wt_idx, which=which, use_graph=False)
    for k in ("energy_history", "fitness_history", "best_idx", "best_step"):
        assert np.array_equal(res[k], res2[k]), k
    assert np.array_equal(tr["flat"], tr2["flat"]) and np.array_equal(tr["accepted"], tr2["accepted"])
    # the way bench.py issues it: no trace buffers (the specialised chain kernels), graph replay, either evaluation policy
    for reuse in (False, True):
        _, _, res3 = _philox_run(m, n, T, 2, 10, False, i0, Lp, wt_idx, which=which, trace=False, reuse_grad=reuse, use_graph=True)
        for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
            assert np.array_equal(res[k], res3[k]), (reuse, k)


def test_config2_composition_against_the_oracle():
    """BASELINE config 2 exactly as bench.py runs it -- 128 chains, Potts-only product of experts (which = 1), PABP geometry,
    no mutation cap, device RNG, re-evaluating policy, hipGraph replay, no trace buffers: the stand-alone Potts kernel and the
    specialised k_propose / k_accept instantiations -- against the oracle fed with the device's own noise (T = 20)."""
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    n, T, pas, Lp = 128, 20, 2, J.shape[0]
    ch, tr, res = _philox_run(m, n, T, pas, 0, False, i0, Lp, wt_idx, which=1, reuse_grad=False, use_graph=False)
    from helpers import device_noise
    noise = device_noise(ch, T, pas)
    en = oracle_energy(J, h, i0, wt_idx, None, 0.0)
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, 0, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert (res["fitness_history"] == 0).all()                                  # no supervised expert in this energy
    for reuse in (False, True):                                                 # the untraced, graph-replayed runs bench.py times
        ch3, _, res3 = _philox_run(m, n, T, pas, 0, False, i0, Lp, wt_idx, which=1, trace=False, reuse_grad=reuse, use_graph=True)
        assert ch3.graph_stats()["replayed_steps"] == T
        for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
            assert np.array_equal(res[k], res3[k]), (reuse, k)


@pytest.mark.parametrize("weights", ["seeded", "trained"])
def test_config3_composition_against_the_oracle(weights):
    """BASELINE config 3 exactly as bench.py runs it -- 128 chains, Potts + supervised CNN product of experts (which = 3,
    lamda = 5), PABP geometry, no mutation cap, device RNG: the fused experts launch and the chain kernels -- against the oracle
    fed with the device's own noise (T = 20), on the seeded networks and on the shipped checkpoints' values. Draws, accept bits
    and best states exact; energies at this file's e_tol + 4e-6 * lamda * max(1, |fit|); the untraced graph-replayed runs
    bench.py times, under both evaluation policies, bit-equal to the traced run."""
    fx, J, h, i0, wt_idx, cnn, m = _philox_setup()
    lam = 5.0
    if weights == "trained":
        from helpers import real_pabp_cnn_states
        cnn = real_pabp_cnn_states()[0]
        m = hip_model(J, h, i0, wt_idx, cnn, lam)
    n, T, pas, Lp = 128, 20, 2, J.shape[0]
    ch, tr, res = _philox_run(m, n, T, pas, 0, False, i0, Lp, wt_idx, which=3, reuse_grad=False, use_graph=False)
    from helpers import device_noise
    noise = device_noise(ch, T, pas)
    en = oracle_energy(J, h, i0, wt_idx, cnn, lam)
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, 0, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    eh, fh = ref["energy_history"].numpy(), ref["fitness_history"].numpy()
    assert observed(f"config3_composition_{weights}:energy_history", np.abs(res["energy_history"] - eh),
                    e_tol(eh, lam) + 4e-6 * lam * np.maximum(1.0, np.abs(fh))) <= 1.0
    assert observed(f"config3_composition_{weights}:fitness_history", np.abs(res["fitness_history"] - fh), 5e-6 * np.maximum(1.0, np.abs(fh))) <= 1.0
    for reuse in (False, True):                                                 # the untraced, graph-replayed runs bench.py times
        ch3, _, res3 = _philox_run(m, n, T, pas, 0, False, i0, Lp, wt_idx, which=3, trace=False, reuse_grad=reuse, use_graph=True)
        assert ch3.graph_stats()["replayed_steps"] == T
        for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
            assert np.array_equal(res[k], res3[k]), (reuse, k)


def test_one_dominant_move_keeps_the_normaliser_conditioned():
    """One gradient entry ~50 above the rest of its row (a field h[l0][k0] of +50): the first sub-step takes that move with
    probability ~1 and the residue that held all the softmax mass then holds none -- carrying the normaliser across sub-steps
    as S1 += (new - old) cancels to rounding noise there (true remainder L * 20 * exp(-25) ~ 3e-8 against ulp(1) = 6e-8), so
    the device path re-sums it (pas.h propose_body_dev). Paths of up to five moves, device RNG, oracle fed the device's noise:
    every draw after the dominant move, the forward / reverse log-probabilities (accept bits) and the energies must agree."""
    from helpers import device_noise
    fx, J, h, i0, wt_idx, cnn, m0 = _philox_setup()
    Lp = J.shape[0]
    l0 = 37
    k0 = (int(wt_idx[i0 + l0]) + 7) % 20
    h = h.copy()
    h[l0, k0] += 50.0
    m = hip_model(J, h, i0, wt_idx, None, 0.0)
    n, T, pas = 32, 12, 3
    for reuse in (False, True):
        ch, tr, res = _philox_run(m, n, T, pas, 0, False, i0, Lp, wt_idx, which=1, reuse_grad=reuse, use_graph=False)
        noise = device_noise(ch, T, pas)
        en = oracle_energy(J, h, i0, wt_idx, None, 0.0)
        ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, 0, False, trace=True)
        dominant = 0
        for t in range(T):
            U = noise[t][0].numpy()
            for s in range(int(U.max())):
                act = s < U
                assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (reuse, t, s)
                dominant += int(((tr["flat"][t, s] == (i0 + l0) * 20 + k0) & (s + 1 < U)).sum())
        assert dominant >= n // 3                  # the dominant move was taken with sub-steps still to come, many times
        assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
        eh = ref["energy_history"].numpy()
        assert observed(f"dominant_move:energy_history:reuse{int(reuse)}", np.abs(res["energy_history"] - eh), e_tol(eh)) <= 1.0
        assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())


def test_error_paths():
    """The reference's only runtime failure on this path is torch.distributions' ValueError on an undefined categorical
    (every move masked out); the HIP path reports the same condition. API misuse returns errors instead of faulting."""
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    fx = load("ops_toy24_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = hip_model(J, h, i0, wt_idx, cnn, 5.0)
    Lp = J.shape[0]
    # a chain at the mutation cap whose only mutation lies outside [min_pos, max_pos]: no admissible move at all
    start = np.tile(wt_idx, (4, 1))
    start[:, 0] = (wt_idx[0] + 1) % 20
    ch = Chains(m, 4, 3, 2, 1, False, i0, i0 + Lp - 1, 3, 1, seed=1)
    ch.init(torch.as_tensor(start).cuda())
    ch.run(1)
    with pytest.raises(ValueError):
        ch.sync()
    ch2 = Chains(m, 4, 3, 2, 0, False, i0, i0 + Lp - 1, 3, 1, seed=1)
    ch2.init(torch.as_tensor(start).cuda())
    with pytest.raises(PpdeHipError):
        ch2.run(5)                                   # beyond max_steps
    with pytest.raises(PpdeHipError):
        Chains(m, 4, 3, 2, 0, False, 5, 2, 3, 1)     # min_pos > max_pos
    with pytest.raises(PpdeHipError):
        m.energy_grad(torch.zeros(2, 24, dtype=torch.uint8).cuda(), 7)
    with pytest.raises(ValueError):
        m.onehot_to_idx(torch.zeros(2, 23, 20).cuda())


def test_long_replay_stays_on_the_oracle_trajectory():
    """300 iterations x 16 chains (about 10k categorical draws, 4.8k accept decisions) on host-drawn noise: the HIP path
    stays on the oracle's trajectory to the end -- draws can only differ on ~1e-6-wide near-ties."""
    fx = load("ops_pabp_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    lam, n, T, pas, nmut = 5.0, 16, 300, 2, 6
    Lp, L = J.shape[0], wt_idx.shape[0]
    torch.manual_seed(2024)
    noise = [orc.draw_noise_torch(n, L * 20, pas) for _ in range(T)]
    en = oracle_energy(J, h, i0, wt_idx, cnn, lam)
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, nmut, False)
    from ppde_amd.sampler import Chains
    m = hip_model(J, h, i0, wt_idx, cnn, lam)
    ch = Chains(m, n, T, pas, nmut, False, i0, i0 + Lp - 1, 3, 0, trace=True, random_chain=3)
    ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    _feed(ch, noise, n)
    tr, res = ch.trace(), ch.collect()
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 3].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 5e-5


def test_masked_entry_winning_the_race_keeps_the_clamp_probability():
    """clamp_probs leaves every masked entry with probability 2^-23, so with a narrow proposal range a masked move wins
    the exponential race now and then; its forward log-probability is log(2^-23 / sum), not that of its unmasked logit
    (found by tests/fuzz_sampler.py). Device RNG, oracle fed with the device's noise."""
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    from ppde_amd import synthetic
    L, Lp, i0, n, T, pas, lo, hi = 64, 4, 49, 128, 40, 3, 29, 36
    wt = np.random.default_rng(19).integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=19)
    m = HipModel(wt, "cuda:0"); m.set_potts(J, h, i0); m.set_lamda(0.0)
    ch = Chains(m, n, T, pas, 0, False, lo, hi, 1, 1, trace=True, random_chain=0, seed=1020, use_graph=False)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = []
    for t in range(T):
        qs = [ch.philox_dump(t, s) for s in range(2 * pas - 1)]
        noise.append((qs[-1][2].cpu().long(), torch.stack([q[0].cpu() for q in qs], 0), qs[-1][1].cpu()))
    en = oracle_energy(J, h, i0, wt, None, 0.0)
    ref = orc.run(en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, lo, hi, pas, 0, False, trace=True)
    outside = 0
    for t in range(T):
        U = noise[t][0].numpy()
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
            res_idx = tr["flat"][t, s][act] // 20
            outside += int(((res_idx < lo) | (res_idx > hi)).sum())
        assert np.allclose(tr["log_acc"][t], ref["traces"][t]["log_acc"].numpy(), atol=2e-4), t
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert outside >= 1, "the configuration no longer exercises a masked winner"

"""The C ABI's declared shape limits (include/ppde_hip.h) at their edges, on the GPU, against the fp64 references of
tests/helpers_limits.py: the supervised expert across n_nets / C / K / F / L (A), the Potts kernel at the windows the ring
kernel with 8 chunk groups serves and deep inside long sequences (B), chains at L = 307 and ppde_pas_length = 64 (C), and the
refusals (D). Everything goes through HipModel / Chains, i.e. through the C ABI. tests/test_abi_limits_cpu.py has validated the
references and the inputs (tie-free: no chain is exempted here) and defines err32; budgets: helpers_limits docstring."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_limits as hl
import ppde_oracle as orc
from helpers import device_noise, oracle_energy
from test_hip_parity import e_tol, observed
from ppde_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNN_NAMES = [c["name"] for c in hl.CNN_CASES]
POTTS_NAMES = [c["name"] for c in hl.POTTS_CASES]


def _hold(case, r, e, f, g):
    """every chain's energy / fitness / gradient within the case's budget of the fp64 reference; ratios recorded, printed first"""
    ratios = {}
    for k, dev, ref in (("e", e, r["e"]), ("fit", f, r["fit"]), ("grad", g, r["g"])):
        if dev is None:
            continue
        err = np.abs(np.asarray(dev, dtype=np.float64) - ref)
        if k == "grad":
            err = err.reshape(err.shape[0], -1).max(1)
        ratios[k] = observed(f"limits:{case}:{k}", err, r["budget"][k])
    print(f"[limits] {case}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + (f"; 4 x err32 budget for {r['branch']}" if r["branch"] else "; project tolerances"), flush=True)
    assert all(np.isfinite(v) and v <= 1.0 for v in ratios.values()), (case, ratios)
    return ratios


def _cnn_model(c):
    from ppde_amd.energy import HipModel
    m = HipModel(c["wt"], "cuda:0")
    if c["J"] is not None:
        m.set_potts(c["J"], c["h"], c["i0"])
    m.set_cnn(c["states"])
    m.set_lamda(c["lam"])
    return m


# ---- A. the supervised expert across its declared shape space --------------------------------------------------------------
@pytest.mark.parametrize("name", CNN_NAMES)
def test_supervised_expert_at_the_declared_shapes(name):
    c, r = hl.build_cnn_case(name), hl.cnn_case_reference(name)
    print(f"[limits] {name}: L={c['L']} C={c['C']} K={c['K']} F={c['F']} n_nets={c['nets']} n={c['n']} potts={c['potts']} which={c['which']} "
          f"lam={c['lam']} seed={hl.CNN_SEEDS.get(name, 0)} -- {c['form']}", flush=True)          # before the launch: a fault names its case
    m = _cnn_model(c)
    x = torch.as_tensor(c["idx"]).cuda()
    e, f, g = m.energy_grad(x, c["which"])
    _hold(name, r, e.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy())
    e2, f2, g2 = m.energy_grad(x, c["which"], want_grad=False)                                  # grad_dev = NULL: no backward
    assert g2 is None
    _hold(name + ":nograd", r, e2.cpu().numpy(), f2.cpu().numpy(), None)
    m.close()


_CHUNKED_BY_KNOB = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
import helpers_limits as hl
from test_abi_limits_gpu import _cnn_model
out = {}
for name in ("ube4b_nets1", "ube4b_nets4"):
    c = hl.build_cnn_case(name)
    print("[limits] chunked by knob:", name, flush=True)
    m = _cnn_model(c)
    e, f, g = m.energy_grad(torch.as_tensor(c["idx"]).cuda(), 2)
    out["e_" + name], out["f_" + name], out["g_" + name] = e.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy()
    m.close()
np.savez(sys.argv[2], **out)
"""


def test_ube4b_pinned_chunk_backward_with_one_and_four_networks():
    """launch_cnn picks the UBE4B-pinned backward chunk kernel (shape == 1) by T / CP / F alone; the shape itself is served by the
    single-launch kernel today, so the chunk kernels are selected with the library's own knob PPDE_CNN_CHUNKED=1 (read once per
    process, hence the child process): one and four networks against fp64."""
    with tempfile.TemporaryDirectory() as d:
        script, out = os.path.join(d, "chunked.py"), os.path.join(d, "out.npz")
        open(script, "w").write(_CHUNKED_BY_KNOB)
        sys.stdout.flush()
        # the child writes to this process's stdout / stderr: the case it names before each launch is on record whether it
        # fails, faults or runs into the time limit
        p = subprocess.run([sys.executable, script, REPO, out], timeout=300, env=dict(os.environ, PPDE_CNN_CHUNKED="1"))
        assert p.returncode == 0, p.returncode
        res = dict(np.load(out))
    for name in ("ube4b_nets1", "ube4b_nets4"):
        _hold(name + ":chunked", hl.cnn_case_reference(name), res["e_" + name], res["f_" + name], res["g_" + name])


# ---- B. Potts beyond what has run --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POTTS_NAMES)
def test_potts_windows_beyond_what_has_run(name):
    from ppde_amd.energy import HipModel
    c, r = hl.build_potts_case(name), hl.potts_case_reference(name)
    print(f"[limits] {name}: L={c['L']} Lp={c['Lp']} i0={c['i0']} n={c['n']} which=1 NC={(((c['Lp'] + 3) // 4) + 3) // 4}", flush=True)
    m = HipModel(c["wt"], "cuda:0")
    m.set_potts(c["J"], c["h"], c["i0"])
    e, f, g = m.energy_grad(torch.as_tensor(c["idx"]).cuda(), 1)
    e, f, g = e.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy()
    outside = np.ones(c["L"], bool)
    outside[c["i0"]:c["i0"] + c["Lp"]] = False
    assert not np.any(g[:, outside]) and not np.any(f), "the gradient outside the window and the fitness of a Potts-only energy are exact zeros"
    rr = dict(r, budget={k: v for k, v in r["budget"].items() if k != "fit"})
    _hold(name, rr, e, None, g)
    # H(wt) against its own fp64 value, held to its own budget (the oracle's H(wt) is the measuring stick, not dH's)
    ratio = observed(f"limits:{name}:H_wt", abs(m.wt_hamiltonian - r["H_wt"]), r["budget"]["H_wt"])
    print(f"[limits] {name}: H_wt {ratio:.3f}" + ("; 4 x err32 budget" if "H_wt" in r["branch"] else "; project tolerance"), flush=True)
    assert ratio <= 1.0, (m.wt_hamiltonian, r["H_wt"])
    m.close()


# ---- C. chains at their limits -----------------------------------------------------------------------------------------------
def _exact_against_oracle(ch, en, wt, n, T, pas, lo, hi, nmut, lam, tag):
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    ref = orc.run(en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, lo, hi, pas, nmut, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    eh = ref["energy_history"].numpy()
    assert observed(f"limits:{tag}:energy_history", np.abs(res["energy_history"] - eh), e_tol(eh, lam)) <= 1.0
    return res


@pytest.mark.parametrize("with_cnn", [False, True])
def test_chains_at_the_longest_sequence_they_take(with_cnn):
    """L = 307 (the 6140 proposal logits of a chain fill the registers of its workgroup: ppde_chains_create), Potts window 120 .. 183,
    device RNG, eagerly and replayed from the captured graph: draws, accept bits and best states exact, energies within e_tol."""
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    L, Lp, i0, n, T, pas, nmut = 307, 64, 120, 8, 4, 2, 4
    lam = 2.0 if with_cnn else 0.0
    rng = np.random.default_rng(307)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=307, symmetric=False)
    cnn = [hl.make_cnn(32, 5, 64, 300 + s) for s in range(3)] if with_cnn else None
    which = 3 if with_cnn else 1
    print(f"[limits] chains L={L} Lp={Lp} i0={i0} n={n} T={T} pas={pas} which={which} cnn={'C=32 F=64 K=5 x3 (chunked: 5 forward chunks)' if with_cnn else None}", flush=True)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    if cnn:
        m.set_cnn(cnn)
    m.set_lamda(lam)
    en = oracle_energy(J, h, i0, wt, cnn, lam)
    results = []
    for graph in (False, True):
        ch = Chains(m, n, T, pas, nmut, False, i0, i0 + Lp - 1, which, 1, seed=9, trace=True, random_chain=0, use_graph=graph)
        ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
        ch.run(T)
        results.append(_exact_against_oracle(ch, en, wt, n, T, pas, i0, i0 + Lp - 1, nmut, lam, f"chains_L307_{'cnn' if with_cnn else 'potts'}_{'graph' if graph else 'eager'}"))
        ch.close()
    for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
        assert np.array_equal(results[0][k], results[1][k]), k
    m.close()


@pytest.mark.parametrize("rng_mode", [1, 0])
def test_chains_at_pas_length_64(rng_mode):
    """ppde_pas_length = 64: paths of up to 127 moves. U within [1, 127], trace entries beyond U are -1, and against the oracle on
    the same noise: draws and accept bits equal up to a chain's first difference, which must be a near-tie of the oracle's own
    decision (race gap <= 1e-5, |log_acc - log u| <= 2e-4 U / 5); at most 2 of the 16 chains may part."""
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    p = hl.PAS64
    n, T, pas = p["n"], p["T"], p["pas"]
    wt, J, h, i0, Lp, cnn = hl.pas64_model()
    L = wt.shape[0]
    print(f"[limits] chains pas={pas} L={L} Lp={Lp} i0={i0} n={n} T={T} nmut=0 which=3 rng_mode={rng_mode}", flush=True)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    m.set_cnn(cnn)
    m.set_lamda(p["lam"])
    ch = Chains(m, n, T, pas, p["nmut"], False, i0, i0 + Lp - 1, 3, rng_mode, seed=p["seed"], trace=True, random_chain=0)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    if rng_mode == 1:
        ch.run(T)
        noise = device_noise(ch, T, pas)
    else:
        torch.manual_seed(64)
        noise = [orc.draw_noise_torch(n, L * 20, pas) for _ in range(T)]
        for U, q, u in noise:
            ch.run(1, (U.to(torch.int32).reshape(1, -1), q, u.reshape(1, -1), [int(q.shape[0])]))
    tr = ch.trace()
    U = np.stack([nz[0].numpy() for nz in noise])
    assert np.array_equal(tr["U"], U) and U.min() >= 1 and U.max() <= 2 * pas - 1 and U.max() > pas
    steps = np.arange(2 * pas - 1)[None, :, None]
    beyond = steps >= U[:, None, :]
    assert np.all(tr["flat"][beyond] == -1) and np.all(tr["flat"][~beyond] >= 0) and np.all(tr["flat"][~beyond] < L * 20)
    ref = hl.pas64_oracle_run(noise)
    n_same, notes, same = hl.compare_pas64(tr, ref, noise)
    print(f"[limits] pas64 rng_mode={rng_mode}: {n_same}/{n} chains on the oracle's trajectory to the end; near-ties: {notes}", flush=True)
    assert n_same >= n - 2
    # log_acc of the chains that stayed (a parted chain is on another trajectory from there on)
    la_ref = np.stack([ref["traces"][t]["log_acc"].numpy() for t in range(T)])
    finite = np.isfinite(la_ref[:, same]) & np.isfinite(tr["log_acc"][:, same])
    err = np.where(finite, np.abs(tr["log_acc"][:, same] - la_ref[:, same]), 0.0)
    assert np.array_equal(np.isfinite(la_ref[:, same]), np.isfinite(tr["log_acc"][:, same]))
    assert observed(f"limits:pas64_rng{rng_mode}:log_acc", err, hl.pas64_acc_tol(U[:, same])) <= 1.0
    res = ch.collect()
    eh = ref["energy_history"].numpy()[:, same]
    assert observed(f"limits:pas64_rng{rng_mode}:energy_history", np.abs(res["energy_history"][:, same] - eh), e_tol(eh, p["lam"])) <= 1.0
    ch.close()
    m.close()


# ---- D. refusals: PPDE_ERR_INVALID with a message, and the object stays usable -----------------------------------------------
def _refused(fn, *words):
    from ppde_amd._hip import PpdeHipError
    with pytest.raises(PpdeHipError) as ei:
        fn()
    msg = str(ei.value)
    assert msg.startswith("[-1] ") and len(msg) > len("[-1] "), msg                       # PPDE_ERR_INVALID and a non-empty message
    for w in words:
        assert w in msg, (w, msg)
    return msg


def _raw_set_cnn(m, n_nets, Cc, K, F):
    """ppde_model_set_cnn with any numbers (HipModel.set_cnn reads them off the arrays): zero arrays of the declared sizes"""
    from ppde_amd import _hip
    k = max(n_nets, 1)
    arrs = dict(cw=np.zeros(max(Cc * 20 * K, 1), np.float32), cb=np.zeros(max(Cc, 1), np.float32), lw=np.zeros(max(F * Cc, 1), np.float32),
                lb=np.zeros(max(F, 1), np.float32), dw=np.zeros(max(F, 1), np.float32), db=np.zeros(1, np.float32))
    ptrs = {key: (C.c_void_p * k)(*[a.ctypes.data] * k) for key, a in arrs.items()}
    _hip.check(m.lib.ppde_model_set_cnn(m.handle, n_nets, Cc, K, F, *[ptrs[key] for key in ("cw", "cb", "lw", "lb", "dw", "db")]))


def test_model_length_limits():
    from ppde_amd.energy import HipModel
    _refused(lambda: HipModel(np.zeros(4, np.uint8), "cuda:0"), "length")
    _refused(lambda: HipModel(np.zeros(4097, np.uint8), "cuda:0"), "length")
    for L in (5, 4096):
        HipModel(np.zeros(L, np.uint8), "cuda:0").close()


def test_set_cnn_refusals_leave_the_expert_that_was_there():
    from ppde_amd.energy import HipModel
    c, r = hl.build_cnn_case("C33_F33"), hl.cnn_case_reference("C33_F33")
    m = _cnn_model(c)
    x = torch.as_tensor(c["idx"]).cuda()
    before = [t.cpu().numpy() for t in m.energy_grad(x, 2)]
    L = c["L"]
    for nets, Cc, K, F in ((0, 8, 5, 16), (5, 8, 5, 16), (3, 8, 0, 16), (3, 8, 9, 16), (3, 0, 5, 16), (3, 8, 5, 0)):
        _refused(lambda: _raw_set_cnn(m, nets, Cc, K, F))
    # a width past the chunk kernels' LDS: C = 1024 at L = 40 (neither launch form holds 1024 channels); the message names channels
    msg = _refused(lambda: _raw_set_cnn(m, 3, 1024, 5, 64), "channels", "1024")
    assert "sequence too long" not in msg
    # more features than the backward window's route bitmap has room for (FP <= 32 * max(CP, 20 * taps) = 3200 here)
    _refused(lambda: _raw_set_cnn(m, 3, 32, 5, 3201), "features", "3200")
    after = [t.cpu().numpy() for t in m.energy_grad(x, 2)]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    _hold("refusals:cnn_still_usable", r, *after)
    m.close()
    m8 = HipModel(np.zeros(8, np.uint8), "cuda:0")
    _refused(lambda: _raw_set_cnn(m8, 3, 8, 8 + 1, 16))                                    # K 9
    m7 = HipModel(np.zeros(7, np.uint8), "cuda:0")
    _refused(lambda: _raw_set_cnn(m7, 3, 8, 8, 16))                                        # K > L with K itself legal
    _raw_set_cnn(m7, 3, 8, 7, 16)                                                          # K = L is the edge: accepted
    m7.close(); m8.close()


def test_reference_shaped_network_one_step_past_the_edge_is_refused_at_set_cnn():
    """L = 545: CP = 576, the backward chunk kernel would need 165824 of 163840 bytes (helpers_limits, ref_L544): refused by
    ppde_model_set_cnn, where the shape is known, in channels; L = 544 (the ref_L544 case) is served."""
    from ppde_amd.energy import HipModel
    L = 545
    m = HipModel(np.zeros(L, np.uint8), "cuda:0")
    msg = _refused(lambda: m.set_cnn([hl.make_cnn(L, 5, 2 * L, s) for s in range(3)]), "channels", "545", "544")
    assert "sequence too long" not in msg
    assert not m.has_cnn
    _refused(lambda: m.energy_grad(torch.zeros(1, L, dtype=torch.uint8).cuda(), 2), "supervised")
    m.set_cnn([hl.make_cnn(32, 5, 64, s) for s in range(3)])                                   # the model is still usable
    e, f, g = m.energy_grad(torch.zeros(2, L, dtype=torch.uint8).cuda(), 2)
    fo, go = hl.cnn_fp64([hl.make_cnn(32, 5, 64, s) for s in range(3)], np.zeros((2, L), np.uint8))
    ratio = observed("limits:refusals:L545_then_C32:fit", np.abs(f.cpu().numpy() - fo), 5e-6 * np.maximum(1.0, np.abs(fo)))
    print(f"[limits] refusals: L=545, C=32 F=64 after the refusal: fit {ratio:.3f}; project tolerance", flush=True)
    assert ratio <= 1.0, ratio
    m.close()


def test_potts_window_of_513_is_refused_before_the_model_is_touched():
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    L = 520
    rng = np.random.default_rng(520)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    m = HipModel(wt, "cuda:0")
    J64, h64 = synthetic.make_potts(64, seed=5, symmetric=False)
    m.set_potts(J64, h64, 100)
    idx = hl.make_rows(wt, 4, rng)
    x = torch.as_tensor(idx).cuda()
    before = [t.cpu().numpy() for t in m.energy_grad(x, 1)]
    wt_H = m.wt_hamiltonian
    _refused(lambda: m.set_potts(np.zeros((513, 513, 20, 20), np.float32), np.zeros((513, 20), np.float32), 0), "512")
    # refused before the model was touched: the expert that was there still answers, bit for bit
    after = [t.cpu().numpy() for t in m.energy_grad(x, 1)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and m.wt_hamiltonian == wt_H
    m.close()
    # on a model WITHOUT a Potts expert the refusal leaves none: evaluation and chains fail cleanly, a valid window then works
    m = HipModel(wt, "cuda:0")
    _refused(lambda: m.set_potts(np.zeros((513, 513, 20, 20), np.float32), np.zeros((513, 20), np.float32), 0), "512")
    assert not m.has_potts
    _refused(lambda: m.energy_grad(x, 1), "Potts")
    _refused(lambda: Chains(m, 4, 2, 2, 0, False, 0, L - 1, 1, 1), "Potts")
    _refused(lambda: m.wt_hamiltonian, "Potts")
    m.set_potts(J64, h64, 100)
    e, f, g = [t.cpu().numpy() for t in m.energy_grad(x, 1)]
    assert all(np.array_equal(a, b) for a, b in zip(before, (e, f, g)))
    eo, go = hl.potts_fp64(J64, h64, 100, wt, idx)
    ratios = [observed("limits:refusals:potts_after_513:e", np.abs(e - eo), 5e-6 * np.maximum(1.0, np.abs(eo))),
              observed("limits:refusals:potts_after_513:grad", np.abs(g - go), 2e-6 * max(1.0, np.abs(go).max()))]
    print(f"[limits] refusals: Lp=64 at 100 of 520 after the refusal: e {ratios[0]:.3f}, grad {ratios[1]:.3f}; project tolerances", flush=True)
    assert max(ratios) <= 1.0, ratios
    m.close()


def test_chain_limits():
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    J, h = synthetic.make_potts(16, seed=1)
    m = HipModel(np.zeros(308, np.uint8), "cuda:0")
    m.set_potts(J, h, 4)
    _refused(lambda: Chains(m, 4, 2, 2, 0, False, 4, 19, 1, 1), "307")
    e, _, _ = m.energy_grad(torch.zeros(2, 308, dtype=torch.uint8).cuda(), 1)                  # the model itself serves L = 308
    assert np.abs(e.cpu().numpy()).max() <= 5e-6                                               # dH of the wild type
    m.close()
    m = HipModel(np.zeros(24, np.uint8), "cuda:0")
    m.set_potts(J, h, 4)
    _refused(lambda: Chains(m, 4, 2, 0, 0, False, 4, 19, 1, 1), "pas_length")
    _refused(lambda: Chains(m, 4, 2, 65, 0, False, 4, 19, 1, 1), "pas_length")
    ch = Chains(m, 4, 2, 64, 0, False, 4, 19, 1, 1, seed=3)                                    # and a valid object afterwards runs
    ch.init(torch.zeros(4, 24, dtype=torch.uint8).cuda())
    ch.run(2)
    assert np.isfinite(ch.collect()["energy_history"]).all()
    ch.close()
    m.close()

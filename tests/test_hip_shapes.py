"""GPU parity at the other proteins' shapes (BASELINE.json configs 4/5 sizes) and odd geometries: every kernel
instantiation (chain groups per thread, Potts chunk counts, CNN row tiles, padded convolution taps) against the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppde_oracle as orc
from helpers import oracle_energy, vet_gradient_outliers
from test_hip_parity import e_tol, observed
from ppde_amd import synthetic
from ppde_amd.encoding import seqs_to_idx


def _model(L, Lp, i0, with_cnn, lam, seed=5, K=5):
    from ppde_amd.energy import HipModel
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, symmetric=False)
    cnn = None
    if with_cnn:
        cnn = [synthetic.make_cnn_state(L, s, kernel_size=K) for s in range(3)]
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    if cnn:
        m.set_cnn(cnn)
    m.set_lamda(lam)
    return m, wt, J, h, cnn


@pytest.mark.parametrize("L,Lp,i0,with_cnn", [(237, 237, 0, True),       # GFP with its CNN: the chunked long-sequence kernels
                                               (150, 60, 20, True), (133, 133, 0, True),
                                               (237, 237, 0, False),      # GFP: window = whole protein
                                               (104, 76, 23, True),       # UBE4B: odd window start
                                               (237, 100, 77, False), (40, 7, 31, True), (24, 16, 4, True),
                                               (300, 120, 50, True)])     # more than 512 CNN features, ring Potts not needed
def test_energy_grad_shapes(L, Lp, i0, with_cnn):
    lam = 3.0 if with_cnn else 0.0
    m, wt, J, h, cnn = _model(L, Lp, i0, with_cnn, lam)
    en = oracle_energy(J, h, i0, wt, cnn, lam)
    rng = np.random.default_rng(L)
    idx = np.tile(wt, (20, 1))
    for b in range(20):
        pos = rng.choice(L, size=min(L, b), replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    which = 3 if with_cnn else 1
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), which)
    eo, fo, go = en.energy_grad(torch.as_tensor(idx.astype(np.int64)))
    # SURVEY 8(c)'s tolerances (the oracle is pinned to the reference at the same ones): energies 5e-6 * max(1, |e|) plus the
    # fitness term's 4e-6 * lamda * max(1, |fit|), fitness 5e-6, gradients 2e-6 * max(1, lamda) relative to the largest entry
    tag = f"shape_L{L}_Lp{Lp}_i{i0}_{'cnn' if with_cnn else 'potts'}"
    eo_, fo_, go_ = eo.numpy(), fo.numpy(), go.numpy()
    assert observed(tag + ":e", np.abs(e.cpu().numpy() - eo_), e_tol(eo_) + 4e-6 * lam * np.maximum(1.0, np.abs(fo_))) <= 1.0
    assert observed(tag + ":fit", np.abs(f.cpu().numpy() - fo_), 5e-6 * np.maximum(1.0, np.abs(fo_))) <= 1.0
    # the max over t picks a row: where two rows tie to within matmul rounding the routed gradient is implementation-defined
    # (numerics contract); a chain over the tolerance must then sit, within the same tolerance, on the gradient of
    # another admissible routing (helpers.classify_chain_gradient; the 300-residue case holds such a chain: network 1, feature
    # 413, rows 200 / 168, relative gap 4.5e-7). Only chains whose routing cannot be read off the gradient are left out.
    gtol = 2e-6 * max(1.0, lam) * max(1.0, float(np.abs(go_).max()))
    gc = en.cnn.fit_grad(torch.as_tensor(idx.astype(np.int64)))[1].numpy() if with_cnn else None
    dg, unresolved = vet_gradient_outliers(g.cpu().numpy(), go_, gc, cnn, idx, gtol, lamda=lam, label=tag)
    keep = np.setdiff1d(np.arange(idx.shape[0]), unresolved)
    assert observed(tag + ":grad", dg[keep], gtol) <= 1.0, (dg, gtol)


@pytest.mark.parametrize("L,K", [(50, 3), (150, 3), (278, 3), (120, 7)])
def test_cnn_other_kernel_size(L, K):
    """kernel sizes other than 5 go through the zero-padded 8-tap instantiation, single-launch and chunked
    (278 x 3: found by tests/fuzz_energy_grad.py, the forward chunk read letters of rows it had not staged)"""
    m, wt, J, h, cnn = _model(L, 30, 10, True, 2.0, K=K)
    en = oracle_energy(J, h, 10, wt, cnn, 2.0)
    idx = np.random.default_rng(0).integers(0, 20, (6, L)).astype(np.uint8)
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 2)
    fo, go = en.cnn.fit_grad(torch.as_tensor(idx.astype(np.int64)))
    assert observed(f"cnn_L{L}_K{K}:fit", np.abs(f.cpu().numpy() - fo.numpy()), 5e-6 * np.maximum(1.0, np.abs(fo.numpy()))) <= 1.0
    assert observed(f"cnn_L{L}_K{K}:grad", np.abs(g.cpu().numpy() - go.numpy()).max(), 2e-6 * max(1.0, float(go.abs().max()))) <= 1.0


def _rescaled(cnn, enc, emb, dec, spread=0):
    """the synthetic networks with their layers multiplied by enc / emb / dec, and (spread > 0) channel c of the first layer by
    2^e_c with the second layer's column c by 2^-e_c, e_c cycling through -spread .. spread: the same function, operands of very
    different magnitudes from channel to channel"""
    out = []
    for st in cnn:
        st = {k: np.array(v, dtype=np.float32) for k, v in st.items()}
        C = st["encoder.weight"].shape[0]
        ec = (np.arange(C) % (2 * spread + 1)) - spread if spread else np.zeros(C)
        sc = np.exp2(ec).astype(np.float32)
        st["encoder.weight"] = st["encoder.weight"] * np.float32(enc) * sc[:, None, None]
        st["encoder.bias"] = st["encoder.bias"] * np.float32(enc) * sc
        st["embedding.0.weight"] = st["embedding.0.weight"] * np.float32(emb) / sc[None, :]
        st["embedding.0.bias"] = st["embedding.0.bias"] * np.float32(enc * emb)
        st["decoder.weight"] = st["decoder.weight"] * np.float32(dec)
        out.append(st)
    return out


@pytest.mark.parametrize("L", [96, 150])             # single launch (matrix-pipe convolution) / chunked (table gather)
@pytest.mark.parametrize("enc,emb,dec,spread", [(1e-3, 1.0, 1.0, 0), (40.0, 1e-2, 100.0, 0), (1e3, 1e3, 1e-5, 0), (1e-4, 1e-3, 1e6, 0),
                                                (1.0, 1.0, 1.0, 6), (1.0, 1.0, 1.0, 12)])
def test_cnn_weight_magnitudes(L, enc, emb, dec, spread):
    """The split-precision contractions scale their operands by powers of two from static bounds (fp16 terms have five exponent
    bits): networks whose layers sit orders of magnitude away from the trained ones', and whose channels differ by up to 2^24 in
    magnitude among themselves, against the oracle, errors relative to the outputs' own scale."""
    from ppde_amd.energy import HipModel
    rng = np.random.default_rng(7)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    cnn = _rescaled([synthetic.make_cnn_state(L, s) for s in range(3)], enc, emb, dec, spread)
    J, h = synthetic.make_potts(30, seed=3, symmetric=True)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, 10)
    m.set_cnn(cnn)
    m.set_lamda(2.0)
    en = oracle_energy(J, h, 10, wt, cnn, 2.0)
    idx = rng.integers(0, 20, (24, L)).astype(np.uint8)
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 2)
    fo, go = en.cnn.fit_grad(torch.as_tensor(idx.astype(np.int64)))
    fo_, go_ = fo.numpy(), go.numpy()
    tag = f"magnitudes_L{L}_{enc:g}_{emb:g}_{dec:g}_s{spread}"
    fscale = max(float(np.abs(fo_).max()), 1e-30)
    gscale = max(float(np.abs(go_).max()), 1e-30)
    assert observed(tag + ":fit", np.abs(f.cpu().numpy() - fo_), 5e-6 * fscale) <= 1.0
    # (which = 2: the gradient is d fit / d x itself; a chain over the tolerance must sit on another admissible vertex)
    dg, unresolved = vet_gradient_outliers(g.cpu().numpy(), go_, go_, cnn, idx, 4e-6 * gscale, lamda=1.0, label=tag)
    keep = np.setdiff1d(np.arange(idx.shape[0]), unresolved)
    assert observed(tag + ":grad", dg[keep], 4e-6 * gscale) <= 1.0, (dg / gscale, unresolved)


@pytest.mark.parametrize("L,Lp,i0,n,with_cnn", [(237, 237, 0, 24, False), (237, 237, 0, 6, True), (104, 76, 23, 20, True),
                                                 (40, 7, 31, 1, True), (300, 120, 50, 6, False)])
def test_sampler_vs_oracle_shapes(L, Lp, i0, n, with_cnn):
    """Trajectories at GFP / UBE4B sizes and with a single chain, host-drawn noise into both implementations."""
    from ppde_amd.sampler import Chains
    lam = 2.0 if with_cnn else 0.0
    m, wt, J, h, cnn = _model(L, Lp, i0, with_cnn, lam)
    en = oracle_energy(J, h, i0, wt, cnn, lam)
    T, pas, nmut = 12, 2, 4
    torch.manual_seed(L + n)
    noise = [orc.draw_noise_torch(n, L * 20, pas) for _ in range(T)]
    ref = orc.run(en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, nmut, False, trace=True)
    ch = Chains(m, n, T, pas, nmut, False, i0, i0 + Lp - 1, 3 if with_cnn else 1, 0, trace=True, random_chain=0)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q, u.reshape(1, -1), [int(q.shape[0])]))
    tr, res = ch.trace(), ch.collect()
    for t in range(T):
        U = noise[t][0].numpy()
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 1e-4
    # and the device-RNG path at this shape (graph + fused kernels; one to four race waves, one to three groups per thread)
    # against the oracle fed with the device's own noise -- the two-level draw, the fixed softmax reference, the reverse path
    from helpers import device_noise
    T2 = 45
    ch2 = Chains(m, n, T2, pas, nmut, False, i0, i0 + Lp - 1, 3 if with_cnn else 1, 1, seed=4, trace=True, random_chain=0)
    ch2.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch2.run(T2)
    tr2, r2 = ch2.trace(), ch2.collect()
    assert np.isfinite(r2["energy_history"]).all() and np.array_equal(r2["best_energy"], r2["energy_history"].max(0))
    noise2 = device_noise(ch2, T2, pas)
    ref2 = orc.run(en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise2[t], T2, i0, i0 + Lp - 1, pas, nmut, False, trace=True)
    for t in range(T2):
        U = noise2[t][0].numpy()
        assert np.array_equal(tr2["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr2["flat"][t, s][act], ref2["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr2["accepted"].astype(bool), ref2["accepted"].numpy())
    assert np.array_equal(r2["best_idx"], ref2["best_idx"].numpy())
    assert np.abs(r2["energy_history"] - ref2["energy_history"].numpy()).max() <= 1e-4
    # the same run without trace buffers (specialised kernels, graph replay) gives the same bits
    ch3 = Chains(m, n, T2, pas, nmut, False, i0, i0 + Lp - 1, 3 if with_cnn else 1, 1, seed=4, random_chain=0)
    ch3.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch3.run(T2)
    r3 = ch3.collect()
    for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
        assert np.array_equal(r2[k], r3[k]), k


@pytest.mark.parametrize("L,Lp,i0,with_cnn,n", [(237, 237, 0, False, 300),    # ring Potts kernel, 2 chain groups, 3 chain blocks
                                                 (96, 80, 8, True, 100),       # both experts in one launch (2 chain groups)
                                                 (96, 80, 8, True, 300),       # several chain blocks of two groups in the fused launch
                                                 (104, 76, 23, True, 70),      # one single-launch CNN workgroup per CU would fit: chunked CNN instead
                                                 (237, 237, 0, True, 70)])     # chunked CNN + ring Potts
def test_batch_composition_does_not_change_a_bit(L, Lp, i0, with_cnn, n):
    """Every chain's energy, fitness and gradient are bit-identical whether it is evaluated in a large batch (other
    chain-group counts, other launch shapes, other kernels) or in batches of 20: results cannot depend on sharding."""
    lam = 3.0 if with_cnn else 0.0
    m, wt, J, h, cnn = _model(L, Lp, i0, with_cnn, lam)
    rng = np.random.default_rng(n)
    idx = np.tile(wt, (n, 1))
    for b in range(n):
        pos = rng.choice(L, size=min(L, b % 17), replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    which = 3 if with_cnn else 1
    x = torch.as_tensor(idx).cuda()
    e, f, g = m.energy_grad(x, which)
    for lo in range(0, n, 20):
        e2, f2, g2 = m.energy_grad(x[lo:lo + 20], which)
        assert torch.equal(e[lo:lo + 20], e2) and torch.equal(f[lo:lo + 20], f2) and torch.equal(g[lo:lo + 20], g2), lo


_POTTS_WINDOWS = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_hip_shapes import _model
out = {}
for Lp in (1, 3, 16, 17, 33, 50, 64, 65, 80, 97, 113, 128, 129, 145, 161, 180, 200, 210, 237, 241, 256, 260):
    L = Lp + 9
    m, wt, J, h, _ = _model(L, Lp, 4, False, 0.0, seed=Lp)
    for n in (5, 70, 130):
        idx = np.random.default_rng(Lp + n).integers(0, 20, (n, L)).astype(np.uint8)
        e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 1)
        out[f"e_{Lp}_{n}"], out[f"g_{Lp}_{n}"] = e.cpu().numpy(), g.cpu().numpy()
    m.close()
np.savez(sys.argv[2], **out)
"""


def test_potts_instantiations_with_pinned_chunk_count_equal_the_general_kernels():
    """Every Potts window of up to 256 residues runs an instantiation with its chunk count (1..16) as a compile-time constant
    (potts.h NCC), resident slab and ring alike; PPDE_POTTS_SPEC=0 selects the general kernels (run-time chunk count), which
    also serve longer windows. Same summation order: energies and gradients must be bit-identical (22 window lengths on both
    sides of every chunk boundary, three batch sizes = one / two chain groups, ragged)."""
    import os
    import subprocess
    import sys
    import tempfile
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "windows.py")
        open(script, "w").write(_POTTS_WINDOWS)
        for spec in ("1", "0"):
            out = os.path.join(d, f"spec{spec}.npz")
            r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=400,
                               env=dict(os.environ, PPDE_POTTS_SPEC=spec))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            res[spec] = dict(np.load(out))
    assert len(res["1"]) == 2 * 22 * 3
    for k in res["1"]:
        assert np.isfinite(res["1"][k]).all() and np.array_equal(res["1"][k], res["0"][k]), k


_CNN_KNOBS = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_hip_shapes import _model
out = {}
for (L, Lp, i0) in ((96, 80, 8), (104, 76, 23), (237, 237, 0)):
    m, wt, J, h, cnn = _model(L, Lp, i0, True, 3.0, seed=L)
    for n in (3, 130):
        idx = np.random.default_rng(L + n).integers(0, 20, (n, L)).astype(np.uint8)
        idx[0] = wt
        e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 3)
        out[f"e_{L}_{n}"], out[f"f_{L}_{n}"], out[f"g_{L}_{n}"] = e.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy()
    m.close()
np.savez(sys.argv[2], **out)
"""


def test_cnn_launch_forms_give_the_same_bits():
    """The supervised expert's kernels in their pinned (PPDE_CNN_SPEC, default) and general instantiations, fused with the Potts
    tiles in one launch (default) or launched separately (PPDE_FUSE_EXPERTS=0), the long proteins' chunk kernels with 512 (default
    above 128 channels) or 256 threads (PPDE_CNN_CHUNK_512=0): same arithmetic, so energies, fitness and
    gradients must be bit-identical at the PABP (single launch), UBE4B and GFP (chunked) shapes."""
    import os
    import subprocess
    import sys
    import tempfile
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "cnn_knobs.py")
        open(script, "w").write(_CNN_KNOBS)
        for tag, env in (("default", {}), ("general", {"PPDE_CNN_SPEC": "0"}), ("unfused", {"PPDE_FUSE_EXPERTS": "0"}),
                         ("chunks256", {"PPDE_CNN_CHUNK_512": "0"})):    # GFP's chunk kernels with 256 threads (default above 128 channels: 512)
            out = os.path.join(d, tag + ".npz")
            r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=400, env=dict(os.environ, **env))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            res[tag] = dict(np.load(out))
    assert len(res["default"]) == 3 * 3 * 2
    for tag in ("general", "unfused", "chunks256"):
        for k in res["default"]:
            assert np.isfinite(res["default"][k]).all() and np.array_equal(res["default"][k], res[tag][k]), (tag, k)


@pytest.mark.parametrize("protein,reps", [("PABP", 3000), ("PABP-trained", 2000), ("UBE4B", 1000), ("GFP", 500)])
def test_repeated_evaluations_are_bit_identical(protein, reps):
    """One evaluation of all experts repeated on the same states must give the same bits every time: a kernel whose result depends
    on timing (a race between waves, a read of memory no one wrote) shows up as a mismatch in some repetition. The states are the
    ones of scripts/probes/repeat_eval.py: among them chains whose half unit routes features into fewer than 49 rows, so the
    compacted backward contraction takes its three-tile instantiation as well as the four- and five-tile ones (a build with
    register spills in that kernel failed exactly there, a few times in 3000 repetitions; the shipped build must never). UBE4B
    runs the general instantiation of the fused launch (seven row tiles), GFP the chunk kernels; the trained PABP networks route
    their features into few rows (the one- and two-tile instantiations)."""
    from ppde_amd.encoding import seqs_to_idx
    from ppde_amd.energy import HipModel
    name = [k for k in synthetic.PROTEINS if k.startswith(protein.split("-")[0])][0]
    _, seq, (i0, Lp) = synthetic.PROTEINS[name]
    wt = seqs_to_idx([seq])[0]
    J, h = synthetic.make_potts(Lp, seed=1234)
    if protein.endswith("-trained"):      # the shipped checkpoints' values: 20-40 features per row, so one or two row tiles in the backward
        from helpers import real_cnn_states
        cnn = real_cnn_states(protein.split("-")[0].lower())[0]
    else:
        cnn = [synthetic.make_cnn_state(len(seq), s) for s in range(3)]
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    m.set_cnn(cnn)
    m.set_lamda(5.0)
    n = 128 if protein.startswith("PABP") else 48
    rng = np.random.default_rng(11)
    idx = np.tile(wt, (n, 1))
    for b in range(n):
        pos = rng.choice(len(wt), size=b % 17, replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    x = torch.as_tensor(idx).cuda()
    e0, f0, g0 = [t.cpu().numpy().copy() for t in m.energy_grad(x, 3)]
    assert np.isfinite(g0).all() and np.isfinite(e0).all()
    # against the oracle once, so that "identical" cannot mean "identically wrong"
    en = oracle_energy(J, h, i0, wt, cnn, 5.0)
    eo, fo, go = en.energy_grad(torch.as_tensor(idx.astype(np.int64)))
    assert np.abs(f0 - fo.numpy()).max() <= 5e-6
    dg = np.abs(g0 - go.numpy()).reshape(n, -1).max(1)
    gtol = 2e-6 * 5.0 * max(1.0, float(go.abs().max()))
    # (a chain over the tolerance must sit on the gradient of another admissible routing of a NEAR tie: DESIGN.md section 5)
    gc = en.cnn.fit_grad(torch.as_tensor(idx.astype(np.int64)))[1].numpy()
    dg, unresolved = vet_gradient_outliers(g0, go.numpy(), gc, cnn, idx, gtol, lamda=5.0, label=f"repeat_{protein}")
    assert dg[np.setdiff1d(np.arange(n), unresolved)].max() <= gtol
    for rep in range(reps):
        e, f, g = [t.cpu().numpy() for t in m.energy_grad(x, 3)]
        assert np.array_equal(e, e0) and np.array_equal(f, f0) and np.array_equal(g, g0), rep

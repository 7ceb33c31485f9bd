"""GPU parity of the transformer unsupervised expert (BASELINE config 5) against oracle/esm_oracle.py.

The reference's model is the third-party esm_one_hot ESM-2 with hub weights, neither of which is in the mount; the oracle
restates the published architecture on self-generated seeded weights, and is pinned to an independent ESM-2 port on those
weights (see its header; tests/test_esm_port_cpu.py). The fork itself and the real checkpoints' values stay open.
Tolerances (fp16 matmuls with fp32 accumulation on both sides, fp16 tensors at the same places): scores
2e-3 * (1 + |s|) ... the observed ratios are appended to gpurun_out/parity_observed.json."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import esm_oracle as eo
from ppde_amd import _hip, synthetic
from ppde_amd.encoding import seqs_to_idx
from test_hip_parity import observed


def _model(L, layers, dim, heads, ffn, seed=3, with_cnn=False, potts=None, state=None):
    """`state`: the transformer's weights, where they are not make_esm2_state's of `seed` (the rescaled ones of the range tests)."""
    from ppde_amd.energy import HipModel
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=seed) if state is None else state
    m = HipModel(wt, "cuda:0")
    if potts:
        J, h = synthetic.make_potts(potts[1], seed=seed)
        m.set_potts(J, h, potts[0])
    cnn = None
    if with_cnn:
        cnn = [synthetic.make_cnn_state(L, s) for s in range(3)]
        m.set_cnn(cnn)
    m.set_transformer(st, heads)
    return m, wt, st, cnn


def _read(m, what, layer, shape):
    out = np.empty(int(np.prod(shape)), np.float32)
    _hip.check(m.lib.ppde_debug_transformer_read(m.handle, what, layer, _hip.ptr(out), out.size))
    return out.reshape(shape)


@pytest.mark.parametrize("L,layers,dim,heads,ffn,n", [(24, 2, 128, 4, 256, 5),        # toy
                                                       (104, 30, 640, 20, 2560, 3),     # esm2_t30_150M shapes, UBE4B length
                                                       (128, 2, 128, 4, 256, 3),        # the 128-residue attention kernels, full
                                                       (129, 2, 128, 4, 256, 2),        # the 256-residue kernels, one row past 128
                                                       (237, 3, 256, 8, 512, 3),        # GFP length: two passes over the key halves
                                                       (256, 2, 128, 4, 256, 2),        # the longest sequence supported
                                                       (24, 2, 256, 4, 512, 4),         # head width 64, toy
                                                       (128, 2, 256, 4, 512, 2),        # head width 64, full length
                                                       (237, 2, 256, 4, 512, 2),        # head width 64, GFP length (rows-only LDS image, four passes)
                                                       (256, 2, 128, 2, 256, 2),        # head width 64, the longest sequence
                                                       (104, 33, 1280, 20, 5120, 2),    # esm2_t33_650M shapes (transformer-L)
                                                       (24, 2, 96, 4, 256, 4),          # head width 24 (rows padded 96 -> 128), toy
                                                       (237, 2, 96, 4, 256, 2),         # head width 24, GFP length
                                                       (104, 12, 480, 20, 1920, 3)])    # esm2_t12_35M shapes (transformer-S)
def test_score_and_gradient_vs_oracle(L, layers, dim, heads, ffn, n):
    m, wt, st, _ = _model(L, layers, dim, heads, ffn)
    orc = eo.EsmOracle(st, layers, dim, heads, half_points=True)
    rng = np.random.default_rng(L)
    idx = np.tile(wt, (n, 1))
    for b in range(1, n):
        pos = rng.choice(L, size=min(L, 3 * b), replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    orc.trace = {}
    s_o, g_o = orc.score_grad(idx.astype(np.int64))
    tr, orc.trace = orc.trace, None
    wt_o = float(orc.score_grad(wt.astype(np.int64)[None])[0][0])
    e, fit, g = m.energy_grad(torch.as_tensor(idx).cuda(), 4)
    # intermediates first: they localise a failure
    M = n * L
    dp = (dim + 127) // 128 * 128                               # device rows are padded to the GEMM tile (480 -> 512), pad columns zero
    for name, what, layer, width, ref in [("x0", 0, 0, 1, tr["xin0"].reshape(M, dim)),
                                          ("qkv0", 1, 0, 3, tr["qkv0"].reshape(M, 3 * dim)),
                                          ("xmid0", 3, 0, 1, tr["xmid0"].reshape(M, dim)),
                                          ("xlast", 5, 0, 1, tr["xlast"].reshape(M, dim))]:
        raw = _read(m, what, layer, (M, width, dp))
        assert not raw[:, :, dim:].any(), name
        got = raw[:, :, :dim].reshape(M, width * dim)
        err = np.abs(got - ref.numpy())
        assert observed(f"tf{layers}:{name}", err.max(), 2e-2 * (1 + np.abs(ref.numpy()).max())) <= 1.0, name
    lg = _read(m, 6, 0, (M, 128))[:, :33]
    assert observed(f"tf{layers}:logits", np.abs(lg - tr["logits"].reshape(M, 33).numpy()).max(), 3e-2 * (1 + tr["logits"].abs().max().item())) <= 1.0
    assert observed(f"tf{layers}:wt_score", abs(m.transformer_wt_score - wt_o), 2e-3 * (1 + abs(wt_o))) <= 1.0
    s_dev = e.cpu().numpy() + m.transformer_wt_score
    assert observed(f"tf{layers}:score", np.abs(s_dev - s_o.numpy()), 2e-3 * (1 + np.abs(s_o.numpy()))) <= 1.0
    assert float(e[0]) == 0.0                                   # the wild type's Delta is exactly zero
    assert float(fit.abs().max()) == 0.0
    gd, go = g.cpu().numpy(), g_o.numpy()
    assert observed(f"tf{layers}:grad", np.abs(gd - go).max(), 3e-2 * np.abs(go).max()) <= 1.0
    # a chain's numbers do not depend on the batch it sits in
    e1, _, g1 = m.energy_grad(torch.as_tensor(idx[1:2]).cuda(), 4)
    assert torch.equal(e1, e[1:2]) and torch.equal(g1, g[1:2])


@pytest.mark.parametrize("L,win", [(24, (4, 16)), (237, (0, 237))])      # toy; GFP length (ring Potts, chunked CNN, 256-residue attention)
def test_product_of_experts_with_transformer_and_sampler(L, win):
    """which = 6 (transformer + supervised CNN) and 7 (potts + transformer + CNN): the energy is the sum of the experts'
    terms; the gradient is the UNSUPERVISED experts' only, as the reference's transformer branch yields (energy.py:125
    differentiates w.r.t. the minibatch slice), and with PPDE_WHICH_FULL_GRAD (bit 3) the sum over all experts. A sampler
    run on the device RNG gives the same trajectory with and without gradient reuse. (Oracle replays of which = 6 / 7 runs:
    test_tfpoe_device_rng_run_vs_oracle, test_tfpoe_sampler_replays_reference_run.)"""
    from ppde_amd.sampler import Chains
    layers, dim, heads, ffn, lam = 2, 128, 4, 256, 2.0
    m, wt, st, cnn = _model(L, layers, dim, heads, ffn, with_cnn=True, potts=win)
    m.set_lamda(lam)
    idx = np.random.default_rng(1).integers(0, 20, (6, L)).astype(np.uint8)
    x = torch.as_tensor(idx).cuda()
    e4, _, g4 = m.energy_grad(x, 4)
    e2, f2, g2 = m.energy_grad(x, 2)
    e1, _, g1 = m.energy_grad(x, 1)
    e6, f6, g6 = m.energy_grad(x, 6)
    e7, f7, g7 = m.energy_grad(x, 7)
    _, _, g6f = m.energy_grad(x, 6 | 8)
    _, _, g7f = m.energy_grad(x, 7 | 8)
    tol = 1e-5 * (1 + float(e4.abs().max()) + float(e1.abs().max()))
    assert torch.allclose(e6, e4 + lam * f2, atol=tol) and torch.allclose(f6, f2, atol=0)
    assert torch.equal(g6, g4)                                  # no lamda * d fit/dx in the reference's grad_x
    assert torch.allclose(g6f, g4 + lam * g2, atol=tol)
    assert torch.allclose(e7, e4 + e1 + lam * f2, atol=2 * tol)
    assert torch.allclose(g7, g4 + g1, atol=2 * tol) and torch.allclose(g7f, g4 + g1 + lam * g2, atol=2 * tol)
    # sampler, device RNG, 10 iterations, both evaluation policies give the same trajectory
    n, T = 6, 10
    res = []
    for reuse in (False, True):
        ch = Chains(m, n, T, 2, 3, False, 0, L - 1, 6, 1, reuse_grad=reuse, random_chain=0, seed=5)
        ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
        ch.run(T)
        res.append(ch.collect())
    assert np.array_equal(res[0]["energy_history"], res[1]["energy_history"]) and np.array_equal(res[0]["best_idx"], res[1]["best_idx"])
    e_wt, f_wt, _ = m.energy_grad(torch.as_tensor(wt[None]).cuda(), 6)
    assert np.isfinite(res[0]["energy_history"]).all() and np.all(res[0]["energy_history"][0] == float(e_wt[0]))
    assert abs(float(e_wt[0]) - lam * float(f_wt[0])) < 1e-6        # wild type: Delta score 0, e = lamda * fit
    assert (res[0]["energy_history"][1:] != res[0]["energy_history"][0]).any()


# ---- the reference's transformer branches (energy.py:110-130) ---------------------------------------------------
# Fixtures: the REFERENCE's ProteinProductOfExperts / PPDE_PAS.run over a stand-in for the absent esm_one_hot that serves
# this repository's own ESM-2 restatement in fp32 (tests/golden/make_golden.py). They pin the glue (what is summed into
# the energy, what the gradient is taken of, minibatching, the sampler on top); the ESM arithmetic is pinned elsewhere (tests/test_esm_port_*.py), and
# the HIP path computes it in fp16 where the CPU reference had fp32, hence the tolerances: scores 2e-3 * (1 + |s|),
# gradients 3e-2 * max|g|; draws / accept bits equal except on flagged near-ties of the oracle's own decision.
def _tfpoe_model(fx, unsup):
    from helpers import esm_from_fixture, model_from_fixture
    from ppde_amd.energy import HipModel
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    st, g, _ = esm_from_fixture(fx, True)
    m = HipModel(wt_idx, "cuda:0")
    if unsup == "potts+transformer":
        m.set_potts(J, h, i0)
    m.set_cnn(cnn)
    m.set_transformer(st, g["heads"])
    m.set_lamda(float(fx["lamda"]))
    return m, wt_idx


def _score_tol(fx, tag, lam, fit):
    raw = np.abs(fx[f"{tag}_unsupervised"]) + abs(float(np.ravel(fx[f"{tag}_wt_score"])[0]))
    return 2 * 2e-3 * (1 + raw) + 5e-6 * lam * (1 + np.abs(fit))


@pytest.mark.parametrize("tag,unsup,which", [("t", "transformer", 6), ("pt", "potts+transformer", 7)])
def test_tfpoe_energy_grad_vs_reference_fixture(tag, unsup, which):
    from helpers import load
    fx = load("ops_tfpoe_toy.npz")
    lam = float(fx["lamda"])
    m, wt_idx = _tfpoe_model(fx, unsup)
    x = torch.as_tensor(fx["idx"]).cuda()
    wt_s = float(np.ravel(fx[f"{tag}_wt_score"])[0])
    assert observed(f"tfpoe_{tag}:wt_score", abs(m.transformer_wt_score - wt_s), 2e-3 * (1 + abs(wt_s))) <= 1.0
    e, fit, g = m.energy_grad(x, which)
    assert np.abs(fit.cpu().numpy() - fx[f"{tag}_fit"]).max() <= 5e-6
    assert observed(f"tfpoe_{tag}:e", np.abs(e.cpu().numpy() - fx[f"{tag}_e"]), _score_tol(fx, tag, lam, fx[f"{tag}_fit"])) <= 1.0
    gref = fx[f"{tag}_grad"]
    gtol = 3e-2 * np.abs(gref).max()
    assert observed(f"tfpoe_{tag}:grad", np.abs(g.cpu().numpy() - gref).max(), gtol) <= 1.0
    # ... and the tolerance tells the reference's gradient from the gradient of the whole energy
    sup = lam * fx["supervised_grad"]
    assert np.abs(g.cpu().numpy() - (gref + sup)).max() > 5 * gtol
    _, _, gf = m.energy_grad(x, which | 8)                      # the opt-in: + lamda * d fit/dx
    assert np.abs(gf.cpu().numpy() - (gref + sup)).max() <= gtol + 2e-6 * lam
    e_un, f_un, g_un = m.energy_grad(x, which & ~2)             # get_unsupervised_expert
    assert observed(f"tfpoe_{tag}:unsupervised", np.abs(e_un.cpu().numpy() - fx[f"{tag}_unsupervised"]), _score_tol(fx, tag, 0.0, 0.0)) <= 1.0
    assert float(f_un.abs().max()) == 0.0 and torch.equal(g_un, g)
    e_ng, f_ng, _ = m.energy_grad(x, which, want_grad=False)    # get_energy
    assert torch.equal(e_ng, e) and torch.equal(f_ng, fit)


@pytest.mark.parametrize("name", ["run_tfpoe_toy_t.npz", "run_tfpoe_toy_pt.npz"])
@pytest.mark.parametrize("reuse", [True, False])
def test_tfpoe_sampler_replays_reference_run(name, reuse):
    """The REFERENCE's PPDE_PAS.run with `--unsupervised_expert transformer` (72 chains: two minibatches per evaluation) and
    `potts+transformer`, replayed by the HIP path on the reference's noise."""
    import ppde_oracle as porc
    from helpers import compare_runs_up_to_near_ties, fixture_noise, load, oracle_energy_from_fixture
    from ppde_amd.sampler import Chains
    fx = load(name)
    unsup = str(fx["unsup"])
    which = 6 if unsup == "transformer" else 7
    m, wt_idx = _tfpoe_model(fx, unsup)
    lam, n, T, pas = float(fx["lamda"]), int(fx["n"]), int(fx["T"]), int(fx["pas"])
    L = wt_idx.shape[0]
    noise, same = fixture_noise(fx, n, L * 20, pas, T)
    if not same:
        pytest.skip("this host's torch CPU exponential_ stream differs from the one the fixture was drawn on")
    kw = dict(num_steps=T, min_pos=int(fx["min_pos"]), max_pos=int(fx["max_pos"]), pas_length=pas, nmut_threshold=int(fx["nmut"]),
              paper_results=bool(fx["paper"]))
    # the fp32 oracle replays the fixture exactly (tests/test_oracle_golden.py); its proposal rows say how close each of
    # the reference's decisions was to a tie
    ref = porc.run(oracle_energy_from_fixture(fx), np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t],
                   trace=True, keep_probs=True, **kw)
    assert np.array_equal(ref["accepted"].numpy(), fx["accepted"])
    ch = Chains(m, n, T, pas, int(fx["nmut"]), bool(fx["paper"]), int(fx["min_pos"]), int(fx["max_pos"]), which, 0,
                reuse_grad=reuse, trace=True, random_chain=int(fx["random_idx"]))
    ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q, u.reshape(1, -1), [int(q.shape[0])]))
    tr, res = ch.trace(), ch.collect()
    n_same, notes, same_mask = compare_runs_up_to_near_ties(tr, ref, noise, gap_tol=5e-2, acc_tol=5e-2)
    print(f"[parity] {name} reuse={reuse}: {n_same}/{n} chains on the reference's trajectory to the end; near-ties: {notes}")
    assert n_same >= n - max(1, n // 10)
    eh, fh = fx["energy_history"][:, same_mask], fx["fitness_history"][:, same_mask]
    assert np.abs(res["fitness_history"][:, same_mask] - fh).max() <= 5e-6
    tol = 2 * 2e-3 * (1 + np.abs(eh - lam * fh) + abs(m.transformer_wt_score)) + 5e-6 * lam * (1 + np.abs(fh))
    assert observed(f"{name}:energy_history", np.abs(res["energy_history"][:, same_mask] - eh), tol) <= 1.0
    assert np.array_equal(res["best_idx"][same_mask], fx["best_idx"][same_mask])
    if same_mask[int(fx["random_idx"])]:
        assert np.array_equal(res["random_traj"], fx["random_traj"])


@pytest.mark.parametrize("which", [6, 7, 6 | 8])
def test_tfpoe_device_rng_run_vs_oracle(which):
    """A which = 6 / 7 sampler run on the device RNG against the oracle (fp16 rounding points, energy.py:110-130 glue incl.
    the reference's gradient; 6 | 8: the opt-in full gradient) fed the device's own noise."""
    import ppde_oracle as porc
    from helpers import compare_runs_up_to_near_ties, device_noise, load, oracle_energy_from_fixture
    from ppde_amd.sampler import Chains
    fx = load("ops_tfpoe_toy.npz")
    unsup = "potts+transformer" if which & 1 else "transformer"
    m, wt_idx = _tfpoe_model(fx, unsup)
    n, T, pas, nmut, L = 24, 12, 2, 4, wt_idx.shape[0]
    lo, hi = (int(fx["win_start"]), int(fx["win_start"]) + int(fx["Lp"]) - 1)
    ch = Chains(m, n, T, pas, nmut, False, lo, hi, which, 1, trace=True, random_chain=0, seed=77, use_graph=False)
    ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    en = oracle_energy_from_fixture(fx, half_points=True, full_grad=bool(which & 8), unsup=unsup)
    ref = porc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, lo, hi, pas, nmut, False,
                   trace=True, keep_probs=True)
    n_same, notes, same_mask = compare_runs_up_to_near_ties(tr, ref, noise, gap_tol=5e-2, acc_tol=5e-2)
    print(f"[parity] which={which}: {n_same}/{n} chains on the oracle's trajectory to the end; near-ties: {notes}")
    assert n_same >= n - max(1, n // 4)       # (every chain that parted did so at a near-tie the comparison above validated; observed 20-24 of 24)
    eh = ref["energy_history"].numpy()[:, same_mask]
    fh = ref["fitness_history"].numpy()[:, same_mask]
    lam = float(fx["lamda"])
    tol = 2 * 2e-3 * (1 + np.abs(eh - lam * fh) + abs(m.transformer_wt_score)) + 5e-6 * lam * (1 + np.abs(fh))
    assert observed(f"tfpoe_run{which}:energy_history", np.abs(res["energy_history"][:, same_mask] - eh), tol) <= 1.0
    assert np.array_equal(res["best_idx"][same_mask], ref["best_idx"].numpy()[same_mask])
    assert 0.02 < tr["accepted"].mean() < 0.98


def test_tfpoe_ube4b_150m_shapes_vs_combined_oracle():
    """One which = 6 evaluation at BASELINE config 5's shapes (UBE4B length, esm2_t30_150M geometry, 3 CNNs) against the
    combined oracle: e = Delta-score + lamda * fit, grad = d Delta-score / dx."""
    import ppde_oracle as porc
    name = [k for k in synthetic.PROTEINS if k.startswith("UBE4B")][0]
    wt = seqs_to_idx([synthetic.PROTEINS[name][1]])[0]
    L, layers, dim, heads, ffn, lam, n = wt.shape[0], 30, 640, 20, 2560, 3.0, 4
    from ppde_amd.energy import HipModel
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=0)
    cnn = [synthetic.make_cnn_state(L, s) for s in range(3)]
    m = HipModel(wt, "cuda:0")
    m.set_cnn(cnn)
    m.set_transformer(st, heads)
    m.set_lamda(lam)
    rng = np.random.default_rng(8)
    idx = np.tile(wt, (n, 1))
    for b in range(1, n):
        pos = rng.choice(L, size=2 * b, replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    en = porc.EnergyOracle(None, porc.CnnOracle(cnn), lam, tf=eo.TransformerDelta(eo.EsmOracle(st, layers, dim, heads, half_points=True), wt))
    eo_, fo, go = en.energy_grad(torch.as_tensor(idx.astype(np.int64)))
    e, fit, g = m.energy_grad(torch.as_tensor(idx).cuda(), 6)
    assert np.abs(fit.cpu().numpy() - fo.numpy()).max() <= 5e-6
    raw = np.abs(eo_.numpy() - lam * fo.numpy()) + abs(en.tf.wt_score)
    assert observed("tfpoe_ube4b_150m:e", np.abs(e.cpu().numpy() - eo_.numpy()), 2 * 2e-3 * (1 + raw) + 5e-6 * lam) <= 1.0
    assert observed("tfpoe_ube4b_150m:grad", np.abs(g.cpu().numpy() - go.numpy()).max(), 3e-2 * np.abs(go.numpy()).max()) <= 1.0
    assert float(e[0]) == float(np.float32(lam) * np.float32(float(fit[0])))   # wild type: Delta score exactly 0 (e = 0 + lamda * fit in fp32)


def test_config5_full_size_properties():
    """BASELINE config 5 at its full size (256 chains, UBE4B length, esm2_t30_150M geometry, three CNNs, lamda = 3), a few
    iterations: properties that need no oracle run. Both evaluation policies give the same bits; the running best is the
    maximum over the history (first index on ties) and the stored best state really has that energy; every chain starts at
    the wild type's energy lamda * fit(wt); the mutation cap holds."""
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    name = [k for k in synthetic.PROTEINS if k.startswith("UBE4B")][0]
    wt = seqs_to_idx([synthetic.PROTEINS[name][1]])[0]
    L, n, T, lam = wt.shape[0], 256, 4, 3.0
    m = HipModel(wt, "cuda:0")
    m.set_cnn([synthetic.make_cnn_state(L, s) for s in range(3)])
    m.set_transformer(synthetic.make_esm2_state(30, 640, 20, 2560, seed=0), 20)
    m.set_lamda(lam)
    res = []
    for reuse in (False, True):
        ch = Chains(m, n, T, 2, 10, False, 0, L - 1, 6, 1, reuse_grad=reuse, random_chain=7, seed=11, trace=True)
        ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
        ch.run(T)
        res.append((ch.collect(), ch.trace(), ch.peek()))
    (a, tra, pka), (b, trb, _) = res
    for k in ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(tra["flat"], trb["flat"]) and np.array_equal(tra["accepted"], trb["accepted"])
    eh = a["energy_history"]
    assert np.isfinite(eh).all() and np.array_equal(a["best_energy"], eh.max(0)) and np.array_equal(a["best_step"], eh.argmax(0))
    e_wt, f_wt, _ = m.energy_grad(torch.as_tensor(wt[None]).cuda(), 6, want_grad=False)
    assert np.all(eh[0] == float(e_wt[0])) and float(e_wt[0]) == float(np.float32(lam) * np.float32(float(f_wt[0])))
    e_b, f_b, _ = m.energy_grad(torch.as_tensor(a["best_idx"]).cuda(), 6, want_grad=False)
    assert np.array_equal(e_b.cpu().numpy(), a["best_energy"]) and np.array_equal(f_b.cpu().numpy(), a["best_fitness"])
    assert (pka["dist"] < 10).all() and 0.0 < tra["accepted"].mean() < 1.0


_CHUNKED = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_transformer_gpu import _model
from ppde_amd.sampler import Chains
m, wt, st, cnn = _model(24, 2, 128, 4, 256, with_cnn=True)
m.set_lamda(2.0)
idx = np.random.default_rng(4).integers(0, 20, (13, 24)).astype(np.uint8)
e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 6)
ch = Chains(m, 13, 8, 2, 3, False, 0, 23, 6, 1, random_chain=0, seed=5)
ch.init(torch.as_tensor(np.tile(wt, (13, 1))).cuda()); ch.run(8)
np.savez(sys.argv[2], e=e.cpu().numpy(), g=g.cpu().numpy(), eh=ch.collect()["energy_history"])
"""


def test_populations_beyond_the_workspace_budget_run_in_chunks():
    """The reference bounds the transformer's activation memory by minibatching (64 chains, energy.py:77, :113-127); here a
    workspace holds as many chains as PPDE_TF_WORK_GB allows and larger populations go through chunk by chunk. A child
    process with a 1 MiB budget (5 toy chains per chunk: 13 chains = 5 + 5 + 3) gives the bits of the one-pass evaluation."""
    import subprocess
    import sys
    from ppde_amd.sampler import Chains
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "chunked.npz")
        script = os.path.join(d, "chunked.py")
        open(script, "w").write(_CHUNKED)
        r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PPDE_TF_WORK_GB="0.001"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got = np.load(out)
    m, wt, st, cnn = _model(24, 2, 128, 4, 256, with_cnn=True)
    m.set_lamda(2.0)
    idx = np.random.default_rng(4).integers(0, 20, (13, 24)).astype(np.uint8)
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 6)
    ch = Chains(m, 13, 8, 2, 3, False, 0, 23, 6, 1, random_chain=0, seed=5)
    ch.init(torch.as_tensor(np.tile(wt, (13, 1))).cuda())
    ch.run(8)
    assert np.array_equal(got["e"], e.cpu().numpy()) and np.array_equal(got["g"], g.cpu().numpy())
    assert np.array_equal(got["eh"], ch.collect()["energy_history"])


_BIG_TILES = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_transformer_gpu import _model
out = {}
for tag, (L, layers, dim, heads, ffn, n) in dict(toy=(24, 2, 128, 4, 256, 13), wide=(104, 2, 640, 20, 2560, 6)).items():
    m, wt, st, _ = _model(L, layers, dim, heads, ffn)
    idx = np.random.default_rng(4).integers(0, 20, (n, L)).astype(np.uint8)
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 4)
    out[tag + "_e"], out[tag + "_g"] = e.cpu().numpy(), g.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def test_opt_in_256_row_gemm_tiles_give_the_same_bits():
    """PPDE_TF_BIG=1 routes every GEMM whose shape allows it through tf_gemm_big (256 x 256 / 256 x 128 tiles, loader /
    storer wave roles, all six epilogues): the k order per output element is that of the default 128 x 128 kernel, so scores
    and gradients are bit-identical (toy shapes and one layer pair at the 150M widths: N = 1920, 640, 2560; K = 640, 2560)."""
    import subprocess
    import sys
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "big.py")
        open(script, "w").write(_BIG_TILES)
        # "0": the 128 x 128 kernel everywhere; "1": tf_gemm_big; "160": tf_gemm160 wherever the shape allows
        for tag, env in (("0", dict(PPDE_TF_BIG="0", PPDE_TF_160="0")), ("1", dict(PPDE_TF_BIG="1", PPDE_TF_160="0")),
                         ("160", dict(PPDE_TF_BIG="0", PPDE_TF_160="1", PPDE_TF_TOUCH="0")),
                         ("160t", dict(PPDE_TF_BIG="0", PPDE_TF_160="1", PPDE_TF_TOUCH="1"))):    # ... with the A rows touched ahead into L2 (the default)
            out = os.path.join(d, f"gemm{tag}.npz")
            r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            res[tag] = dict(np.load(out))
    for k in res["0"]:
        assert np.isfinite(res["0"][k]).all(), k
        for other in ("1", "160", "160t"):
            assert np.array_equal(res["0"][k], res[other][k]), (k, other)


def test_reference_style_energy_object_with_a_checkpoint_file():
    """ProteinProductOfExperts(args) with --unsupervised_expert transformer: weights from a checkpoint file in the
    published format (the reference downloads it into --hub_dir)."""
    import argparse
    from ppde_amd.energy import ProteinProductOfExperts
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        synthetic.write_esm2_checkpoint(os.path.join(root, "hub", "checkpoints", "esm2_t30_150M_UR50D.pt"), 2, 128, 4, 256, seed=2)
        # (a 2-layer stand-in under the 150M file name: dimensions are read from the tensors, the head count from the file's
        # cfg.model Namespace, as facebookresearch/esm does)
        args = argparse.Namespace(energy_lamda=1.0, unsupervised_expert="transformer", protein_weights=root, protein="TOY24",
                                  n_chains=4, device="cuda:0", ppde_rng="philox", hub_dir=os.path.join(root, "hub"))
        ef = ProteinProductOfExperts(args)
        x = ef.wt_onehot.repeat(3, 1, 1)
        e, fit = ef.get_energy(x)
        e2, fit2, g = ef.get_energy_and_grads(x)
        assert torch.equal(e, e2) and g.shape == (3, 24, 20) and torch.isfinite(g).all()
        assert torch.allclose(e, fit, atol=1e-6)            # wild type: Delta score is 0, so e = lamda * fit
        assert float(ef.get_unsupervised_expert(x).abs().max()) == 0.0


def test_driver_with_the_transformer_expert():
    """scripts/directed_evolution.py --unsupervised_expert potts+transformer end to end (toy checkpoint under the 150M
    file name in --hub_dir/checkpoints, as the reference's torch-hub download would leave it)."""
    import contextlib
    import glob
    import importlib.util
    import io
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_tf", os.path.join(REPO, "scripts", "directed_evolution.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    if True:
        with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
            synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
            synthetic.write_esm2_checkpoint(os.path.join(res, "checkpoints", "esm2_t30_150M_UR50D.pt"), 2, 128, 4, 256, seed=2)
            argv = ["--protein_weights", root, "--protein", "TOY24", "--results_path", res, "--hub_dir", res, "--device", "cuda:0",
                    "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--unsupervised_expert", "potts+transformer",
                    "--n_chains", "6", "--n_iters", "12", "--seed", "3", "--log_every", "5", "--energy_lamda", "1", "--ppde_rng", "philox"]
            args = drv.build_parser().parse_args(argv)
            args.ppde_reuse_grad = True
            with contextlib.redirect_stdout(io.StringIO()) as buf:
                out_dir = drv.main(args)
            eh = np.load(os.path.join(out_dir, "energy_history.npy"))
            pop = np.load(os.path.join(out_dir, "population.npy"))
            assert eh.shape == (13, 6) and np.isfinite(eh).all() and pop.shape == (6, 24, 20)
            assert np.array_equal(np.load(os.path.join(out_dir, "energy_scores.npy")), eh.max(0))
            assert "[Iteration 4]" in buf.getvalue()


@pytest.mark.parametrize("tag,unsup,which", [("p", "potts", 3), ("t", "transformer", 6), ("pt", "potts+transformer", 7)])
def test_get_energy_under_autograd_vs_reference_fixture(tag, unsup, which):
    """`get_energy` as the relaxed-categorical baseline uses it (mala_approx.py:69-75): fed straight-through samples that
    belong to an autograd graph, differentiated by the caller. Fixture: the REFERENCE's get_energy on inputs its own
    MALAApprox.straight_through_sample drew, and autograd through it (tests/golden/make_golden.py straight). The gradient
    through get_energy carries every expert's term, also on the transformer branches."""
    from helpers import esm_from_fixture, load, model_from_fixture
    from ppde_amd.energy import HipModel, _HipEnergy
    fx = load("ops_straight_through_toy.npz")
    lam = float(fx[f"{tag}_lamda"])
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = HipModel(wt_idx, "cuda:0")
    if which & 1:
        m.set_potts(J, h, i0)
    m.set_cnn(cnn)
    if which & 4:
        st, g, _ = esm_from_fixture(fx, True)
        m.set_transformer(st, g["heads"])
    m.set_lamda(lam)
    en = _HipEnergy()
    en.model, en.which = m, which
    x = torch.as_tensor(fx[f"{tag}_x"]).cuda().requires_grad_()
    assert float((x.detach() - x.detach().round()).abs().max()) > 0          # (one-hot up to an ulp, not exactly)
    e, fit = en.get_energy(x)
    assert e.requires_grad and fit.requires_grad
    g_e = torch.autograd.grad([e.sum()], [x], retain_graph=True)[0]
    w_e, w_f = torch.as_tensor(fx[f"{tag}_w_e"]).cuda(), torch.as_tensor(fx[f"{tag}_w_fit"]).cuda()
    g_mix = torch.autograd.grad([(w_e * e + w_f * fit).sum()], [x])[0]
    assert np.abs(fit.detach().cpu().numpy() - fx[f"{tag}_fit"]).max() <= 5e-6
    half = bool(which & 4)                                                  # fp16 matmuls on the transformer branches
    e_ref, ge_ref, gm_ref = fx[f"{tag}_e"], fx[f"{tag}_grad_e"], fx[f"{tag}_grad_mix"]
    if half:        # as _score_tol: relative to the RAW scores (state and wild type), whose difference the energy holds
        wt_s = abs(float(np.ravel(load("ops_tfpoe_toy.npz")[f"{tag}_wt_score"])[0]))          # (same stand-in model, same wild type)
        e_tol = 2 * 2e-3 * (1 + np.abs(e_ref - lam * fx[f"{tag}_fit"]) + wt_s)
    else:
        e_tol = 5e-6 * np.maximum(1.0, np.abs(e_ref))
    e_tol = e_tol + 5e-6 * lam * (1 + np.abs(fx[f"{tag}_fit"]))
    g_tol = 3e-2 * np.abs(ge_ref).max() if half else 2e-6 * max(1.0, lam)
    assert observed(f"straight_{tag}:e", np.abs(e.detach().cpu().numpy() - e_ref), e_tol) <= 1.0
    assert observed(f"straight_{tag}:grad_e", np.abs(g_e.cpu().numpy() - ge_ref).max(), g_tol) <= 1.0
    assert observed(f"straight_{tag}:grad_mix", np.abs(g_mix.cpu().numpy() - gm_ref).max(), 1.5 * g_tol + 2e-6) <= 1.0
    # the baseline's own use: straight-through of a relaxed sample; its logit gradient is exactly zero in the reference
    # (the estimator is written (x_soft + x_hard) - x_soft: both paths to x_soft cancel), and so it is here
    assert float(fx[f"{tag}_baseline_logit_grad_absmax"]) == 0.0
    soft = torch.rand(x.shape, device="cuda").requires_grad_()
    hard = torch.nn.functional.one_hot(x.detach().argmax(-1), 20).float()
    e2, _ = en.get_energy((soft + hard) - soft)
    assert float(torch.autograd.grad([e2.sum()], [soft])[0].abs().max()) == 0.0
    # plain tensors: no graph, same numbers; relaxed inputs are refused
    e3, fit3 = en.get_energy(x.detach().round())
    assert not e3.requires_grad and torch.equal(e3, e.detach()) and torch.equal(fit3, fit.detach())
    with pytest.raises(ValueError, match="one-hot"):
        en.get_energy((0.9 * x.detach() + 0.005).requires_grad_())
    m.close()


_ATT_FORMS = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_transformer_gpu import _model
out = {}
for tag, (L, layers, dim, heads, ffn, n) in dict(w32=(104, 2, 256, 8, 512, 5), w64long=(237, 2, 256, 4, 512, 3), w24=(60, 2, 96, 4, 256, 4)).items():
    m, wt, st, _ = _model(L, layers, dim, heads, ffn)
    idx = np.random.default_rng(7).integers(0, 20, (n, L)).astype(np.uint8)
    e, f, g = m.energy_grad(torch.as_tensor(idx).cuda(), 4)
    out[tag + "_e"], out[tag + "_g"] = e.cpu().numpy(), g.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def test_both_forms_of_the_attention_backward_agree():
    """tf_attn_bwd_ko (the default: dK / dV accumulated by key owners, one pass at every size) against tf_attn_bwd
    (PPDE_TF_ATT_KO=0: every wave accumulates dK / dV of all keys; two or four passes beyond 128 residues or at head width 64):
    same forward, same P and dS, a different summation order of dK / dV over the query tiles -- scores equal, gradients equal
    to fp16 rounding of the intermediate tensors (head widths 32, 64 at GFP length, 24)."""
    import subprocess
    import sys
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "forms.py")
        open(script, "w").write(_ATT_FORMS)
        for ko in ("1", "0"):
            out = os.path.join(d, f"ko{ko}.npz")
            r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=300, env=dict(os.environ, PPDE_TF_ATT_KO=ko))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            res[ko] = dict(np.load(out))
    for k in res["1"]:
        a, b = res["1"][k], res["0"][k]
        assert np.isfinite(a).all() and np.isfinite(b).all(), k
        if k.endswith("_e"):
            assert np.array_equal(a, b), k                     # the forward does not depend on the backward's form
        else:
            assert observed(f"attn_forms:{k}", np.abs(a - b).max(), 5e-3 * np.abs(a).max()) <= 1.0, k

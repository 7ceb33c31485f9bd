"""The stage-by-stage fp64 reference of the transformer expert (tests/helpers_transformer.py), checked on the CPU:

  * tied to what is pinned: in fp32 without rounding points and with true fp32 matrices it IS EsmOracle(half_points=False)
    (and so reproduces the reference's frozen t_grad / t_unsupervised of ops_tfpoe_toy.npz); with the rounding points it
    is EsmOracle(half_points=True), stage for stage;
  * the mutation table: faults of the kind a kernel could have, planted into the half-points evaluation of one stage, come
    out at >= 2 x the bound the GPU module applies (bound = 4 x yardstick, yardstick = the unmutated half-points
    evaluation's distance from fp64 in the same measure; the unmutated evaluation sits at 0.25 of the bound by
    construction). Multiples are printed (pytest -s) and quoted in DESIGN section 5."""
import functools

import numpy as np
import pytest
import torch

import esm_oracle as eo
import helpers_transformer as ht
from helpers_transformer import F32, F64, Mut
from ppde_amd import synthetic

TOY = (24, 2, 128, 4, 256)


def _fp16_valued(st):
    return {k: (np.asarray(v, np.float32).astype(np.float16).astype(np.float32) if np.ndim(v) == 2 else v) for k, v in st.items()}


def test_fp32_evaluation_is_the_pinned_oracle_and_reproduces_the_reference_fixture():
    from helpers import esm_from_fixture, load, model_from_fixture
    fx = load("ops_tfpoe_toy.npz")
    st, g, orc = esm_from_fixture(fx, False)
    wt_idx = model_from_fixture(fx)[3]
    P = ht.Params(st, g["layers"], g["dim"], g["heads"], fp16_matrices=False)
    idx = fx["idx"].astype(np.int64)
    out = ht.model(P, idx, F32, half=False)
    s_o, g_o = orc.score_grad(idx)
    # the same operations in the same order: equal to fp32 rounding (a few ulp of the score, of the largest gradient entry)
    assert float((out["score"] - s_o).abs().max()) <= 4 * 2.0 ** -23 * float(s_o.abs().max())
    assert float((out["grad"] - g_o).abs().max()) <= 4 * 2.0 ** -23 * float(g_o.abs().max())
    wt_s = float(ht.model(P, wt_idx[None].astype(np.int64), F32, want_grad=False)["score"][0])
    un, gref = fx["t_unsupervised"], fx["t_grad"]
    assert abs(wt_s - float(np.ravel(fx["t_wt_score"])[0])) <= 1e-5 * (1 + abs(wt_s))
    assert np.all(np.abs(out["score"].numpy() - wt_s - un) <= 2e-5 * np.maximum(1.0, np.abs(un)))          # (the fixture test's bounds)
    assert np.abs(out["grad"].numpy() - gref).max() <= 2e-5 * max(1.0, float(np.abs(gref).max()))


def test_half_points_evaluation_is_the_half_points_oracle_stage_for_stage():
    L, layers, dim, heads, ffn = TOY
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=3)
    _, idx = ht.chains_like_the_parity_test(L, 4)
    orc = eo.EsmOracle(_fp16_valued(st), layers, dim, heads, half_points=True)
    orc.trace = {}
    s_o, g_o = orc.score_grad(idx.astype(np.int64))
    tr = orc.trace
    # (gelu_grad_fp16: the one rounding point of the yardstick that the oracle lacks; see the helper's header)
    out = ht.model(ht.Params(st, layers, dim, heads), idx, F32, half=True, gelu_grad_fp16=False)
    for i in range(layers):
        for k in (f"xin{i}", f"qkv{i}", f"ctx{i}", f"xmid{i}"):
            assert torch.equal(out[k], tr[k]), k
    assert torch.equal(out["xlast"], tr["xlast"]) and torch.equal(out["logits"], tr["logits"])
    assert torch.equal(out["score"], s_o) and torch.equal(out["grad"], g_o)
    # the teacher-forced stages are the same functions the model is made of: fed its own intermediates they return them
    P = ht.Params(st, layers, dim, heads)
    for i in range(layers):
        assert torch.equal(ht.stage_a(P, i, out[f"xin{i}"], F32, True), out[f"qkv{i}"])
        ctx, xmid = ht.stage_b(P, i, out[f"xin{i}"], out[f"qkv{i}"], F32, True)
        assert torch.equal(ctx, out[f"ctx{i}"]) and torch.equal(xmid, out[f"xmid{i}"])
        gp, xn = ht.stage_c(P, i, out[f"xmid{i}"], F32, True)
        assert torch.equal(gp, out[f"gp{i}"]) and torch.equal(xn, out[f"xin{i + 1}"] if i + 1 < layers else out["xlast"])
    assert torch.equal(ht.stage_d(P, out["xlast"], F32, True), out["logits"])
    s, dl = ht.stage_e(P, out["logits"], idx, F32, True)
    assert float((s - out["score"]).abs().max()) <= L * 2.0 ** -24 * float(s.abs().max())      # (another order of an fp32 sum of L terms)
    with_grad = ht.model(P, idx, F32, half=True)
    g = ht.stage_g(P, ht.stage_f(P, with_grad["demb"], F32, True), with_grad["logits"], F32, True)
    assert float((g - with_grad["grad"]).abs().max()) <= 4 * 2.0 ** -23 * float(g.abs().max())


# ---- the mutation table ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup(L, layers, dim=128, heads=4, ffn=256, n=3):
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=3)
    P = ht.Params(st, layers, dim, heads)
    _, idx = ht.chains_like_the_parity_test(L, n)
    return P, idx, ht.model(P, idx, F64), ht.model(P, idx, F32, half=True)


def _stage_b_multiples(L, mut):
    """Per layer: the mutant's distance from fp64 in stage B's measure, in yardsticks (inputs: the half-points model's own
    xin_i and q|k|v_i, fp16-valued as the device's are)."""
    P, idx, _, hm = _setup(L, 2)
    res = []
    for i in range(2):
        xin, qkv = hm[f"xin{i}"], hm[f"qkv{i}"]
        ref = ht.stage_b(P, i, xin, qkv, F64)[1]
        yard = ht.row_rel(ht.stage_b(P, i, xin, qkv, F32, True)[1], ref)
        res.append(ht.row_rel(ht.stage_b(P, i, xin, qkv, F32, True, mut)[1], ref) / yard)
    return res


def _backward_multiples(L, mut):
    """One layer, the whole model under autograd: (gradient, d q|k|v of layer 0) in yardsticks."""
    P, idx, ref, hm = _setup(L, 1)
    mm = ht.model(P, idx, F32, half=True, mut=mut)
    return (ht.chain_rel(mm["grad"], ref["grad"]) / ht.chain_rel(hm["grad"], ref["grad"]),
            ht.slice_rel(mm["dqkv0"], ref["dqkv0"], P.hd, 3) / ht.slice_rel(hm["dqkv0"], ref["dqkv0"], P.hd, 3))


# (label, L, mutant): stage B's check must see these at >= 2 x its bound in layer 0 (where the table's figures were taken) and outside the bound in layer 1
FORWARD = [("queries of the last tile never see key L-1", 129, Mut("tail_no_last_key")),
           ("... in head 0 only", 129, Mut("tail_no_last_key", head=0)),
           ("... in chain 1 only", 129, Mut("tail_no_last_key", chain=1)),
           ("pad keys admitted with score 0 and v 0", 129, Mut("pad_keys")),
           ("pad keys admitted with score 0 and v 0, GFP length", 237, Mut("pad_keys")),
           ("rotary position off by one for rows >= 128", 129, Mut("rope_shift_tail"))]
# (label, L, mutant, which of (gradient, d q|k|v) must see it)
BACKWARD = [("dK without the last query tile", 129, Mut("dk_no_tail"), (0, 1)),
            ("dV without the last query tile", 129, Mut("dv_no_tail"), (0, 1)),
            ("... in head 0 only", 129, Mut("dv_no_tail", head=0), (0, 1)),
            ("... in chain 1 only", 129, Mut("dv_no_tail", chain=1), (0, 1)),
            ("layer-norm backward with the mean held constant", 129, Mut("ln_bwd_mean_const"), (0, 1)),
            ("softmax backward: the row sum misses the partial last key tile", 129, Mut("softmax_bwd_rowsum_no_pad_tile"), (0, 1)),
            ("inverse rotary with the forward's sign on dK", 129, Mut("drot_sign_dk"), (0, 1)),
            ("q scale missing in dQ", 129, Mut("dq_no_scale"), (0, 1))]


def test_unmutated_half_points_model_sits_at_a_quarter_of_every_bound():
    P, idx, ref, hm = _setup(129, 1)
    for k, meas in (("grad", ht.chain_rel), ("demb", ht.chain_rel), ("dqkv0", lambda a, b: ht.slice_rel(a, b, P.hd, 3)),
                    ("score", ht.score_rel), ("logits", ht.row_rel)):
        yard = meas(hm[k], ref[k])
        print(f"[yardstick] L=129 one layer {k}: {yard:.3e}")
        assert 0 < yard < 1e-2, k            # fp16 rounding of a handful of stages, not a disagreement of the two restatements
    for i, r in enumerate(_stage_b_multiples(129, None)):
        assert r == 1.0


@pytest.mark.parametrize("label,L,mut", FORWARD, ids=[f"{m.name}-L{L}-h{m.head}-c{m.chain}" for _, L, m in FORWARD])
def test_forward_mutants_land_outside_stage_b_bound(label, L, mut):
    mult = _stage_b_multiples(L, mut)
    print(f"[mutant] {label} (L = {L}): " + ", ".join(f"layer {i}: {m:.1f} x yardstick" for i, m in enumerate(mult)))
    assert mult[0] >= 2 * ht.MARGIN and mult[1] > ht.MARGIN


@pytest.mark.parametrize("label,L,mut,seen_by", BACKWARD, ids=[f"{m.name}-h{m.head}-c{m.chain}" for _, _, m, _ in BACKWARD])
def test_backward_mutants_land_outside_the_whole_model_bounds(label, L, mut, seen_by):
    mult = _backward_multiples(L, mut)
    print(f"[mutant] {label} (L = {L}, one layer): gradient {mult[0]:.1f}, d q|k|v {mult[1]:.1f} x yardstick")
    for j in seen_by:
        assert mult[j] >= 2 * ht.MARGIN


# ---- the tile walk of the persistent GEMMs, and the population geometries that reach it ---------------------------------
POP = [(g, layers) for g in ht.POPULATIONS for layers in (2, 1)]
#             geometry  N    tile: tiles, tiles at ordinal >= 1, highest ordinal
WALK_TABLE = {("P160", 640, 160): (672, 160, 1), ("P160", 1920, 160): (2016, 1504, 3), ("P160", 1280, 160): (1344, 832, 2),
              ("P160", 128, 128): (210, 0, 0),
              ("P128", 256, 128): (740, 228, 1), ("P128", 768, 128): (2220, 1708, 4), ("P128", 512, 128): (1480, 968, 2),
              ("P128", 128, 128): (370, 0, 0)}


@pytest.mark.parametrize("geom,layers", POP, ids=[f"{g}l{l}" for g, l in POP])
def test_population_geometries_reach_later_tiles_of_every_gemm(geom, layers):
    L, dim, heads, ffn, n = ht.POPULATIONS[geom]
    M_pad = ht.pad_rows(n * L)
    assert M_pad % 640 == 0 and 0 <= M_pad - n * L < 640
    shapes = ht.gemm_shapes(dim, ffn, M_pad)
    assert {s[0] for s in shapes} >= {"qkv", "qkv.bwd", "out_proj", "fc1", "fc1.bwd", "fc2", "fc2.bwd", "head_dense", "logits", "embedding.bwd"}
    assert {s[4] for s in shapes if s[1] != 128} == {"tf_gemm160" if geom == "P160" else "tf_gemm_nt"}
    assert {s[3:] for s in shapes if s[1] == 128} == {(128, "tf_gemm_nt")}
    seen = set()
    for name, N, K, tile, kernel in shapes:
        w = ht.walk(M_pad, N, tile)
        tiles = (M_pad // tile) * (N // tile)
        assert w.grid == min((tiles + 7) & ~7, 512) and len(w.ordinal) == tiles
        assert (w.visits == 1).all(), name                           # every tile exactly once
        assert np.array_equal(w.ordinal, ht.tile_walk(M_pad, N, tile))
        later = w.ordinal >= 1
        assert np.array_equal(w.prev[later] >= 0, np.ones(later.sum(), bool)) and (w.prev[~later] == -1).all()
        assert (w.block[w.prev[later]] == w.block[later]).all() and (w.ordinal[w.prev[later]] == w.ordinal[later] - 1).all()
        assert (tiles, int(later.sum()), int(w.ordinal.max())) == WALK_TABLE[(geom, N, tile)], (name, N)
        if N >= 256:
            assert w.ordinal.max() >= 1, name
        else:
            assert w.ordinal.max() == 0                              # (the vocabulary GEMMs stay at one tile per workgroup)
        seen.add(N)
    assert int(ht.tile_walk(M_pad, 3 * dim, 160 if geom == "P160" else 128).max()) >= 3
    chains, why, missing = ht.select_chains(L, n, dim, ffn)
    assert not missing, missing
    assert chains[0] == 0 and chains[-1] == n - 1 and 10 <= len(chains) <= 16
    reasons = " / ".join(r for c in chains for r in why[c])
    for name, N, K, tile, kernel in shapes:
        for k in range(1, int(ht.tile_walk(M_pad, N, tile).max()) + 1):
            assert f"wholly in ordinal {k} of N = {N}, {tile}-tiles" in reasons
    assert "second tile" in reasons and "straddles" in reasons
    print(f"[walk] {geom}: " + "; ".join(f"chain {c}: {', '.join(why[c])}" for c in chains))


def test_walk_of_the_opt_in_256_row_tiles_and_of_one_workgroup_per_tile():
    """The forms the population test runs in child processes: tf_gemm_big (256 x 128 tiles at P160's widths, at most 256
    workgroups, rows padded to 256) walks too; a grid of one workgroup per tile does not."""
    L, dim, heads, ffn, n = ht.POPULATIONS["P160"]
    M_pad = ht.pad_rows(n * L, use160=False, big=True)
    assert M_pad == n * L == 104 * 256
    for N in (dim, 3 * dim, ffn):
        w = ht.walk(M_pad, N, (256, 128 if N % 256 else 256), cap=256)
        assert (w.visits == 1).all() and w.grid == 256 and w.ordinal.max() >= 1
    M_pad = ht.pad_rows(n * L, use160=False)
    for N in (dim, 3 * dim, ffn):
        w = ht.walk(M_pad, N, 128, cap=1 << 30)
        assert (w.visits == 1).all() and w.ordinal.max() == 0


def test_a_stale_first_k_tile_in_later_tiles_lands_outside_stage_b_bound():
    """Planted fault of the walk: in the later tiles of the N = dim GEMM the first k tile (64 of K) of the output projection
    is multiplied from the rows of the workgroup's previous output tile (its LDS image not yet replaced). At P160's widths,
    three chains (312 rows in 640: 4 x 4 tiles of 160) and a synthetic walk -- four workgroups, each walking one column of
    tiles downwards, so the tiles' ordinal is their row tile -- stage B must see it at >= 2 x its bound. The fixed tolerances
    of test_score_and_gradient_vs_oracle (restated here against the unmutated half-points evaluation, that test's reference)
    are printed next to it."""
    L, dim, heads, ffn, _ = ht.POPULATIONS["P160"]
    n, layers = 3, 2
    M_pad = ht.pad_rows(n * L)
    tiles_n = dim // 160
    v = np.arange((M_pad // 160) * tiles_n)
    w = ht.Walk(v // tiles_n, v * 0, v % tiles_n, np.where(v >= tiles_n, v - tiles_n, -1), v * 0 + 1, tiles_n, M_pad, tiles_n, 160, 160)
    mut = Mut("prev_tile_first_k", walk=w)
    P, idx, ref, hm = _setup(L, layers, dim, heads, ffn, n)
    rows_hit = np.zeros((n, L), bool).reshape(-1)
    rows_hit[160:] = True                                            # rows of ordinal >= 1: part of chain 1, all of chain 2
    rows_hit = torch.as_tensor(rows_hit.reshape(n, L))
    mult = []
    for i in range(layers):
        xin, qkv = hm[f"xin{i}"], hm[f"qkv{i}"]
        r = ht.stage_b(P, i, xin, qkv, F64)[1]
        yard = ht.row_rel(ht.stage_b(P, i, xin, qkv, F32, True)[1], r)
        got = ht.stage_b(P, i, xin, qkv, F32, True, mut)[1]
        assert torch.equal(got[~rows_hit], hm[f"xmid{i}"][~rows_hit])            # rows of first tiles are untouched
        mult.append(ht.row_rel(got, r) / yard)
    print("[mutant] first k tile of the output projection from the previous tile's rows (P160 widths): "
          + ", ".join(f"layer {i}: {m:.1f} x yardstick" for i, m in enumerate(mult)))
    assert mult[0] >= 2 * ht.MARGIN and mult[1] > ht.MARGIN
    # the whole-model parity test's tolerances on the same fault
    mm = ht.model(P, idx, F32, half=True, mut=mut)
    big = lambda t: float(t.abs().max())
    fixed = {"xmid0": big(mm["xmid0"] - hm["xmid0"]) / (2e-2 * (1 + big(hm["xmid0"]))),
             "xlast": big(mm["xlast"] - hm["xlast"]) / (2e-2 * (1 + big(hm["xlast"]))),
             "logits": big(mm["logits"] - hm["logits"]) / (3e-2 * (1 + big(hm["logits"]))),
             "score": float(((mm["score"] - hm["score"]).abs() / (2e-3 * (1 + hm["score"].abs()))).max()),
             "grad": big(mm["grad"] - hm["grad"]) / (3e-2 * big(hm["grad"]))}
    print("[mutant] ... against the fixed tolerances of test_score_and_gradient_vs_oracle: "
          + ", ".join(f"{k} {r:.2f}" for k, r in fixed.items()))
    assert min(fixed.values()) > 1.0                                # (stated, not required: the fixed tolerances see this one too)

"""The inputs and references of the ABI-limit cases (tests/helpers_limits.py), checked without a GPU: for every case the fp32
oracle agrees with the independent fp64 reference within the project's tolerances (which validates both and the inputs), the
case is tie-free (so the GPU module exempts no chain), and err32 = |fp32 oracle - fp64|, the measuring stick of the shapes that
are not the reference's, is what the budgets are built from.

Teeth: a wrong fp64 reference fails the same check at the same tolerances (the two perturbation tests at the end)."""
import numpy as np
import pytest
import torch

import helpers_limits as hl
import ppde_oracle as orc

CNN_NAMES = [c["name"] for c in hl.CNN_CASES]
POTTS_NAMES = [c["name"] for c in hl.POTTS_CASES]


def _assert_oracle_agrees(name, r):
    for k, a, b in (("e", r["e32"], r["e"]), ("fit", r["fit32"], r["fit"]), ("grad", r["g32"], r["g"])):
        err = np.abs(a - b)
        tol = r["tol"][k]
        ratio = float(np.max(err / tol))
        print(f"[limits-cpu] {name}:{k}: err32 {float(err.max()):.3e} = {ratio:.3f} of the tolerance, {float(np.max(err / r['tol'][k])):.3f} of the project's"
              + (" (GPU budget: 4 x err32)" if k in r["branch"] else ""))
        assert ratio <= 1.0, (name, k, float(err.max()), tol)
        # the budget is never below the project tolerance and never above max(project, 4 x err32)
        assert np.all(r["budget"][k] >= r["tol"][k]) and np.all(r["budget"][k] <= np.maximum(r["tol"][k], 4.0 * r["err32"][k]))


@pytest.mark.parametrize("name", CNN_NAMES)
def test_cnn_case_oracle_agrees_with_fp64_and_is_tie_free(name):
    c = hl.build_cnn_case(name)
    assert c["idx"].shape == (c["n"], c["L"]) and np.array_equal(c["idx"][0], c["wt"]) and 2 <= c["n"]
    assert len(c["states"]) == c["nets"] and c["states"][0]["encoder.weight"].shape == (c["C"], 20, c["K"])
    assert c["states"][0]["embedding.0.weight"].shape == (c["F"], c["C"])
    r = hl.cnn_case_reference(name)
    assert np.any(r["g"][0]), "degenerate case: the wild type routes no gradient"
    assert hl.case_is_tie_free(c["states"], c["idx"]), "a near-tie or a ReLU kink: pick another seed (helpers_limits.CNN_SEEDS)"
    _assert_oracle_agrees(name, r)
    if hl.is_reference_shape(c):
        assert not r["branch"]


@pytest.mark.parametrize("name", ["L308", "L512", "L1000", "L4096"])
def test_long_sequence_rows_touch_both_ends_and_a_chunk_boundary(name):
    c = hl.build_cnn_case(name)
    changed = np.nonzero(c["idx"][1] != c["wt"])[0]
    K, L = c["K"], c["L"]
    assert set(range(K)) <= set(changed) and set(range(L - K, L)) <= set(changed) and {62, 63, 64, 65} <= set(changed)


@pytest.mark.parametrize("name", POTTS_NAMES)
def test_potts_case_oracle_agrees_with_fp64(name):
    c = hl.build_potts_case(name)
    r = hl.potts_case_reference(name)
    assert c["idx"].shape == (c["n"], c["L"]) and np.array_equal(c["idx"][0], c["wt"])
    assert r["e"][0] == 0.0 and np.abs(r["e"][1:]).min() > 0.0
    outside = np.ones(c["L"], bool)
    outside[c["i0"]:c["i0"] + c["Lp"]] = False
    assert not np.any(r["g"][:, outside]) and np.all(np.any(r["g"][:, ~outside] != 0.0, axis=(1, 2)))
    _assert_oracle_agrees(name, r)
    print(f"[limits-cpu] {name}:H_wt: err32 {r['err32']['H_wt']:.3e} = {r['err32']['H_wt'] / r['tol']['H_wt']:.3f} of the project's tolerance")
    assert r["err32"]["H_wt"] <= r["tol"]["H_wt"] <= r["budget"]["H_wt"] <= max(r["tol"]["H_wt"], 4.0 * r["err32"]["H_wt"])


def test_potts_fp64_on_an_asymmetric_toy_equals_the_dense_form():
    """the blocked gather against x M x written out densely, J asymmetric (the symmetrisation is the point)"""
    rng = np.random.default_rng(3)
    Lp, L, i0 = 7, 12, 3
    J, h = rng.standard_normal((Lp, Lp, 20, 20)).astype(np.float32), rng.standard_normal((Lp, 20)).astype(np.float32)
    wt, idx = rng.integers(0, 20, L), rng.integers(0, 20, (4, L))
    e, g = hl.potts_fp64(J, h, i0, wt, idx)
    Jd, h = J.astype(np.float64), h.astype(np.float64)

    def H(row):
        w = row[i0:i0 + Lp]
        return 0.5 * sum(0.5 * (Jd[i, j, w[i], w[j]] + Jd[j, i, w[j], w[i]]) for i in range(Lp) for j in range(Lp)) + sum(h[i, w[i]] for i in range(Lp))

    assert np.allclose(e, [H(r) - H(wt) for r in idx], rtol=0, atol=1e-12)
    w = idx[0, i0:i0 + Lp]
    g0 = np.array([[sum(0.5 * (Jd[i, j, k, w[j]] + Jd[j, i, w[j], k]) for j in range(Lp)) + h[i, k] for k in range(20)] for i in range(Lp)])
    assert np.allclose(g[0, i0:i0 + Lp], g0, rtol=0, atol=1e-12) and not np.any(g[0, :i0]) and not np.any(g[0, i0 + Lp:])


def test_cnn_fp64_takes_the_first_row_on_an_exact_tie():
    """two identical K-mers: the gradient lands on the first copy's residues only"""
    st = [hl.make_cnn(6, 3, 9, s) for s in range(2)]
    row = np.array([1, 2, 3, 7, 1, 2, 3, 9], dtype=np.uint8)         # rows 0 and 4 see the same 3-mer
    fit, g = hl.cnn_fp64(st, row[None])
    fo, go = orc.CnnOracle(st).fit_grad(torch.as_tensor(row[None].astype(np.int64)))
    assert abs(fit[0] - float(fo[0])) <= 5e-6 and np.abs(g - go.numpy()).max() <= 2e-6
    from helpers import cnn_grad_decompose
    dec = cnn_grad_decompose(st, row, want_rank=False)
    tied = [i for i in dec["info"] if i[0] == "max" and i[3][:2] == [0, 4]]
    assert tied and all(dec["exact"]) and hl.case_is_tie_free(st, row[None])


# ---- teeth: a subtly wrong reference fails the fp32-vs-fp64 check at the same tolerances ------------------------------------
def test_dropping_the_last_feature_strip_fails_the_check():
    name = "C130_F512"
    c, r = hl.build_cnn_case(name), hl.cnn_case_reference(name)
    cut = [dict(sd) for sd in c["states"]]
    for sd in cut:
        w = np.array(sd["decoder.weight"])
        w[:, -16:] = 0.0                              # the last strip of 16 features contributes nothing
        sd["decoder.weight"] = w
    fit, g = hl.cnn_fp64(cut, c["idx"])
    assert np.max(np.abs(r["fit32"] - fit) / r["tol"]["fit"]) > 1.0 and np.abs(r["g32"] - g).max() / r["tol"]["grad"] > 1.0


def test_zeroing_the_last_16_window_residues_fails_the_check():
    name = "window_at_930_of_1000"
    c, r = hl.build_potts_case(name), hl.potts_case_reference(name)
    J, h = c["J"].copy(), c["h"].copy()
    J[-16:] = 0.0
    J[:, -16:] = 0.0
    h[-16:] = 0.0
    e, g = hl.potts_fp64(J, h, c["i0"], c["wt"], c["idx"])
    assert np.max(np.abs(r["e32"] - e)[1:] / r["tol"]["e"][1:]) > 1.0 and np.abs(r["g32"] - g).max() / r["tol"]["grad"] > 1.0


def test_pas64_oracle_run_against_itself_parts_no_chain():
    """the comparison the GPU module applies at ppde_pas_length = 64, oracle against oracle on the device RNG's noise (restated
    on the CPU, oracle/ppde_oracle.py device_noise): all 16 chains stay, path lengths cover [1, 127]"""
    p = hl.PAS64
    noise = [orc.device_noise(p["seed"], 0, p["n"], t, p["pas"], 24) for t in range(p["T"])]
    U = np.stack([u.numpy() for u, _, _ in noise])
    assert U.min() >= 1 and U.max() <= 127 and U.max() > 64
    ref = hl.pas64_oracle_run(noise)
    n_same, notes, _ = hl.compare_pas64(hl.trace_of(ref, p["T"], 127), ref, noise)
    assert n_same == p["n"] and not notes

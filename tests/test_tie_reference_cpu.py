"""The tie-aware fp64 reference of the supervised CNN's input gradient (helpers.cnn_grad_decompose / cnn_grad_match) on the
directed inputs of tests/test_cnn_ties_gpu.py, without a GPU: the conditions those inputs must meet are proved here.

The max over sequence positions routes each feature's decoder weight to one row. Where two rows tie, the gradient is one of
finitely many admissible ones (the vertices of fixed + one alternative per group); the matcher finds the vertex nearest to a
given gradient by least squares and rounding, and the verdict is always the direct comparison with that evaluated vertex. The
tolerance is the GPU test's: 4e-6 of the chain's own largest gradient entry."""
import numpy as np
import pytest
import torch

import ppde_oracle as orc
from helpers import TIE_PLACEMENTS, cnn_grad_decompose, cnn_grad_match, cnn_grad_vertex, tie_networks, tied_states

CASES = [("pabp", False), ("pabp", True), ("ube4b", True), ("gfp", True)]
N = 130
RTOL = 4e-6


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{'trained' if c[1] else 'seeded'}")
def case(request):
    tag, trained = request.param
    cnn = tie_networks(tag, trained)
    idx, which, _ = tied_states(tag, N)
    _, go = orc.CnnOracle(cnn).fit_grad(torch.as_tensor(idx.astype(np.int64)))
    decs = [cnn_grad_decompose(cnn, idx[b]) for b in range(N)]
    return tag, cnn, idx, which, go.numpy().astype(np.float64), decs


def _matches(g, cnn, row, dec):
    v, picks, unresolved, _ = cnn_grad_match(g, cnn, row, dec=dec)
    return float(np.abs(g - v).max()) <= RTOL * float(np.abs(v).max()), picks, v


def test_inputs_are_resolvable_and_cover_every_placement(case):
    tag, cnn, idx, which, go, decs = case
    covered = np.zeros(len(TIE_PLACEMENTS[tag]), int)
    for b, d in enumerate(decs):
        assert not d["unresolved"], b
        assert d["rank"] == d["columns"], (b, d["rank"], d["columns"])            # full column rank: the routing is readable
        t1, t2, m, _, _ = TIE_PLACEMENTS[tag][which[b]]
        hit = [i for i, (e, inf) in enumerate(zip(d["exact"], d["info"])) if e and inf[0] == "max" and inf[3][0] in range(t1, t1 + m - 4)
               and inf[3][-1] in range(t2, t2 + m - 4)]
        covered[which[b]] += bool(hit)
    print(f"[ties] {tag}: chains with an exact tie per placement {covered.tolist()}, most groups in a chain {max(len(d['groups']) for d in decs)}")
    assert (covered >= 1).all(), covered                                          # every placement ties some feature in some chain
    assert covered.sum() >= N // 2


def test_fp32_oracle_sits_on_the_first_row_vertex(case):
    tag, cnn, idx, which, go, decs = case
    worst = 0.0
    for b, d in enumerate(decs):
        ok, picks, v = _matches(go[b], cnn, idx[b], d)
        worst = max(worst, float(np.abs(go[b] - v).max()) / float(np.abs(v).max()))
        assert ok, (b, worst)
        assert not [i for i, k in enumerate(picks) if k and d["exact"][i]], b     # torch.max: the first row of an exact tie
    print(f"[ties] {tag}: fp32 oracle within {worst:.2e} of its vertex, relative to the chain's largest entry (tolerance {RTOL:.0e})")
    assert worst <= RTOL / 4                                                      # the yardstick leaves the device room


def test_random_vertex_with_noise_is_recovered(case):
    tag, cnn, idx, which, go, decs = case
    rng = np.random.default_rng(5)
    for b, d in enumerate(decs):
        picks = [int(rng.integers(0, len(g))) for g in d["groups"]]
        v = cnn_grad_vertex(d, picks)
        g = v + rng.uniform(-1, 1, v.shape) * 4e-7 * np.abs(v).max()              # fp32-size noise (the oracle's own distance)
        ok, got, v2 = _matches(g, cnn, idx[b], d)
        assert ok and np.abs(v2 - v).max() <= 1e-12 * np.abs(v).max(), b
        # the picks agree wherever the alternatives are distinguishable at all
        for i, (k, k2) in enumerate(zip(picks, got)):
            assert k == k2 or np.abs(d["groups"][i][k] - d["groups"][i][k2]).max() <= 1e-9 * np.abs(v).max(), (b, i)


def _largest_tie(d):
    """(group index, |alt1 - alt0|_inf) of the exact tie whose routing changes the gradient most"""
    sizes = [np.abs(g[1] - g[0]).max() if e else 0.0 for g, e in zip(d["groups"], d["exact"])]
    i = int(np.argmax(sizes))
    return i, float(sizes[i])


@pytest.mark.parametrize("kind", ["mixture", "all_mixtures", "wrong_row", "dropped", "doubled"])
def test_wrong_routings_are_rejected(case, kind):
    """A kernel that splits a tied feature between both rows, sends it to a row outside the tie, drops it or adds it twice gives
    a gradient that matches no vertex. The feature perturbed is the chain's most visible exact tie; chains whose most visible
    tie moves the gradient by less than 10 tolerances cannot show the difference and are counted, not tested."""
    tag, cnn, idx, which, go, decs = case
    tested = 0
    for b, d in enumerate(decs):
        if not any(d["exact"]):
            continue
        i, size = _largest_tie(d)
        first = cnn_grad_vertex(d, [0] * len(d["groups"]))
        tol = RTOL * float(np.abs(first).max())
        if size < 10 * tol:
            continue
        tested += 1
        alt = d["groups"][i]
        if kind == "mixture":
            g = first + 0.5 * (alt[1] - alt[0])
        elif kind == "all_mixtures":
            g = first + sum(0.5 * (grp[1] - grp[0]) for grp, e in zip(d["groups"], d["exact"]) if e)
        elif kind == "wrong_row":                                                  # the tied feature's vector, two rows past the first candidate
            t = d["info"][i][3][0]
            cand = set(d["info"][i][3])
            dst = next(r for r in list(range(t + 2, idx.shape[1] - 5)) + list(range(0, t)) if r not in cand)
            moved = np.zeros_like(alt[0])
            moved[dst:dst + 5] = alt[0][t:t + 5]
            g = first - alt[0] + moved
        elif kind == "dropped":
            g = first - alt[0]
        else:
            g = first + alt[1]
        ok, _, _ = _matches(g, cnn, idx[b], d)
        assert not ok, (b, kind)
    print(f"[ties] {tag} {kind}: rejected in {tested} chains")
    assert tested >= N // 3

"""The transformer expert across the dynamic range of its weights, on the CPU: everything here comes from
tests/helpers_transformer.py (fp64, and the evaluation that rounds to fp16 where the device rounds), nothing from device output.

  * the supported range of each function-preserving rescaling (tests/helpers_tf_range.py: RANGE) is recomputed exponent by
    exponent: inside it the half-points evaluation is finite and every whole-model yardstick stays within 2 x its unit-scale
    value (the "larger of two draws of the same rounding process" half of MARGIN); one step beyond each edge it does not;
  * the bounds keep their teeth there: at both edges of every range, and at the peaked exponents, the bounds that reject a
    mutant of tests/test_transformer_stages_cpu.py at unit scale still reject it, unless the regime itself has removed the
    fault from the function (helpers_tf_range.verdict); the peaked exponents are the largest of which that holds;
  * the peaked cases are peaked under fp64;
  * three planted faults that only these regimes see are invisible at unit scale and rejected in their regime.
Figures are printed (pytest -s) and quoted in DESIGN section 5."""
import functools

import numpy as np
import pytest

import helpers_tf_range as hr
import helpers_transformer as ht
from helpers_transformer import Mut
from test_transformer_stages_cpu import BACKWARD, FORWARD

MUTANTS = [("B", L, m) for _, L, m in FORWARD if L == 129] + [("bwd", L, m) for _, L, m, _ in BACKWARD]
_DIST = {"B": hr.stage_b_distances, "bwd": hr.backward_distances, "E": hr.stage_e_distances}


@functools.lru_cache(maxsize=None)
def _unit(kind, L, mut):
    return _DIST[kind](L, mut)


def _verdict(kind, L, mut, family, exponent):
    return hr.verdict(_DIST[kind](L, mut, family, exponent), _unit(kind, L, mut))


def test_regimes_leave_their_input_alone_and_the_preserving_ones_the_fp64_function():
    st = hr.state("17x128", 2)
    before = {k: np.array(v, copy=True) for k, v in st.items()}
    _, _, ref, _ = hr.evaluate("17x128", 2)
    for fam in hr.PRESERVING + hr.PEAKED_FAMILIES:
        out = hr.regime(st, fam, 3, 2)
        assert all(np.array_equal(st[k], before[k]) for k in st) and set(out) == set(st)
        assert any(not np.array_equal(out[k], st[k]) for k in st), fam
        assert all(np.array_equal(hr.regime(out, fam, -3, 2)[k], st[k]) for k in st), fam           # powers of two: exactly undone
        s = hr.evaluate("17x128", 2, fam, 3)[2]["score"]
        moved = float(((s - ref["score"]).abs() / ref["score"].abs()).max())
        print(f"[regime] {fam} x 2^3: the fp64 score moves by {moved:.2e} of itself")
        # (preserved up to the layer norms' epsilon, 1e-5 against a row variance of 1e-2 and more: parts in a thousand at the most)
        assert (moved < 1e-2) == (fam in hr.PRESERVING), fam


def _edges(family):
    lo = hi = 0
    while lo - 1 >= -hr.SEARCH and hr.admitted(family, lo - 1):
        lo -= 1
    while hi + 1 <= hr.SEARCH and hr.admitted(family, hi + 1):
        hi += 1
    return lo, hi


def _figures(family, e):
    geoms = hr.range_geoms(family)
    out = []
    for g in geoms:
        y, unit = hr.case_yardsticks(g, 2, family, e), hr.case_yardsticks(g, 2)
        out.append(f"{g}: " + ("not finite" if y is None else ", ".join(f"{k} {y[k] / unit[k]:.1f}" for k in hr.ROW_YARDSTICKS)))
    return "; ".join(out) + f"; score over them {hr.pooled_score(geoms, family, e) / hr.pooled_score(geoms):.1f}"


@pytest.mark.parametrize("family", hr.PRESERVING)
def test_supported_range_is_the_recomputed_one(family):
    assert hr.admitted(family, 0)
    lo, hi = _edges(family)
    for e in (lo - 1, lo, hi, hi + 1):
        print(f"[range] {family} 2^{e} ({'inside' if lo <= e <= hi else 'outside'}), x unit-scale yardstick: {_figures(family, e)}")
    assert (lo, hi) == hr.RANGE[family]
    assert -hr.SEARCH < lo and hi < hr.SEARCH                        # an edge was found, not the end of the search
    # one step beyond each edge the criterion fails or the evaluation is not finite (what _edges stopped at)
    assert not hr.admitted(family, lo - 1) and not hr.admitted(family, hi + 1)
    # the widest layer-norm row is no part of the search (its evaluations are the slow ones); the edges hold there too
    if "24x1536" in hr.family_geoms(family):
        assert hr.rows_admitted("24x1536", family, lo) and hr.rows_admitted("24x1536", family, hi)
    if family in hr.OVERFLOW:
        o = hr.OVERFLOW[family]
        assert o > hi
        for g in hr.family_geoms(family):
            assert hr.case_yardsticks(g, 2, family, o) is None, g                        # not finite on every geometry
        assert any(hr.case_yardsticks(g, 2, family, o - 1) is not None for g in hr.family_geoms(family))


def test_the_score_of_two_or_three_chains_is_no_yardstick_to_hold_to_a_factor_of_two():
    """Why model.score enters the criterion pooled: chain for chain and geometry for geometry its largest value leaves 2 x its
    unit-scale value inside every range, with nothing else moving; the pooled value does not."""
    out = 0
    for family in hr.PRESERVING:
        geoms, (lo, hi) = hr.range_geoms(family), hr.RANGE[family]
        for e in range(lo, hi + 1):
            assert hr.pooled_score(geoms, family, e) <= 2.0 * hr.pooled_score(geoms)
            out += sum(hr.case_yardsticks(g, 2, family, e)["model.score"] > 2.0 * hr.case_yardsticks(g, 2)["model.score"] for g in geoms)
    print(f"[range] model.score of one geometry beyond 2 x its unit-scale value inside the ranges: {out} times")
    assert out >= 4


EDGE_CASES = [(f, e) for f in hr.PRESERVING for e in hr.RANGE[f]] + [(f, hr.PEAKED[f]) for f in hr.PEAKED_FAMILIES]


def _escaped(family, exponent, label):
    """The live mutants the bounds do not reject at this regime; everything is printed."""
    out = []
    for kind, L, mut in MUTANTS:
        rejected, live, mult = _verdict(kind, L, mut, family, exponent)
        print(f"[{label}] {family} 2^{exponent} {mut.name} h{mut.head} c{mut.chain}: {' / '.join(f'{m:.1f}' for m in mult)} x yardstick"
              + ("" if live else "  (not live: the regime removes the fault)") + ("" if rejected else "  NOT REJECTED"))
        if live and not rejected:
            out.append(mut)
    return out


@pytest.mark.parametrize("family,exponent", EDGE_CASES, ids=[f"{f}{e}" for f, e in EDGE_CASES])
def test_every_bound_keeps_its_teeth_at_the_edges(family, exponent):
    assert _escaped(family, exponent, "teeth") == []
    # and the table is not hollow there: most of its mutants are still live
    assert sum(_verdict(k, L, m, family, exponent)[1] for k, L, m in MUTANTS) >= len(MUTANTS) - 4


@pytest.mark.parametrize("family", hr.PEAKED_FAMILIES)
def test_peaked_exponent_is_the_largest_that_keeps_the_teeth(family):
    top = hr.PEAKED[family]
    for e in range(1, top):
        assert _escaped(family, e, "peaked") == []
    assert _escaped(family, top + 1, "peaked") != []


PEAKED_CASES = [(g, f, e) for g, f, e in hr.CASES if f in hr.PEAKED]


@pytest.mark.parametrize("geom,family,exponent", PEAKED_CASES, ids=[f"{g}-{f}{e}" for g, f, e in PEAKED_CASES])
def test_peaked_cases_are_peaked_under_fp64(geom, family, exponent):
    got = hr.peakedness(geom, family, exponent)
    print(f"[peaked] {geom} {family} 2^{exponent}: {got}")
    if family == "sharp":
        top, low = got
        assert (top > 0.9).all() and (low < 2.0 ** -14).all()
        unit_top = hr.peakedness(geom, family, 0)[0]
        assert (unit_top < 0.9).any()                                # (and it was not so at unit scale)
    elif family == "head":
        assert got > 50 and hr.peakedness(geom, family, 0) < 50
    else:
        assert got > hr.PEAKED_SHARE[geom] > 4 * hr.peakedness(geom, family, 0)


# ---- three planted faults that only these regimes see ----------------------------------------------------------------------
FTZ, NO_MAX, NO_RESCALE, PLUS_MAX = Mut("attn_ftz"), Mut("lse_no_max"), Mut("online_no_rescale"), Mut("lse_plus_max")


def _worst(kind, L, mut, family=None, exponent=0):
    return max(d / y for y, d, _ in _DIST[kind](L, mut, family, exponent))


@pytest.mark.parametrize("kind,L,mut", [("B", 129, FTZ), ("bwd", 129, FTZ), ("B", 237, FTZ), ("E", 129, NO_MAX), ("E", 17, PLUS_MAX), ("E", 129, PLUS_MAX), ("B", 129, NO_RESCALE),
                                        ("bwd", 129, NO_RESCALE), ("B", 237, NO_RESCALE), ("bwd", 237, NO_RESCALE)],
                         ids=lambda v: v if isinstance(v, str) else (v.name if isinstance(v, Mut) else str(v)))
def test_new_mutants_are_invisible_at_unit_scale(kind, L, mut):
    w = _worst(kind, L, mut)
    print(f"[mutant] {mut.name} at unit scale, L = {L}, {kind}: {w:.2f} x yardstick")
    assert w <= ht.MARGIN / 2                                        # no further out than a second draw of the rounding itself


def test_flushed_fp16_subnormals_are_rejected_at_the_low_edges_of_qk_and_vo():
    """q x 2^-12 and v x 2^-14 put q and v among fp16's subnormals: an attention that reads them as zero loses them. Under `sharp`
    the flushed probabilities (below 2^-14 each, 129 of them at the most) carry less than the rounding of the rest: that fault
    is not one the bounds can see, nor one that matters; the figure is printed."""
    for family in ("qk", "vo"):
        lo = hr.RANGE[family][0]
        w = [d / y for y, d, _ in hr.stage_b_distances(129, FTZ, family, lo)]
        print(f"[mutant] attn_ftz under {family} 2^{lo}: stage B {w[0]:.0f}, {w[1]:.0f} x yardstick")
        assert min(w) >= 2 * ht.MARGIN
        assert _worst("bwd", 129, FTZ, family, lo) >= 2 * ht.MARGIN
    e = hr.PEAKED["sharp"]
    print(f"[mutant] attn_ftz under sharp 2^{e}: stage B {_worst('B', 129, FTZ, 'sharp', e):.2f}, backward {_worst('bwd', 129, FTZ, 'sharp', e):.2f} x yardstick")


def test_log_softmax_without_the_row_maximum_is_rejected_under_head():
    e = hr.PEAKED["head"]
    score, dlogits = (d / y for y, d, _ in hr.stage_e_distances(129, NO_MAX, "head", e))
    print(f"[mutant] lse_no_max under head 2^{e}: score {score:.1f}, d logits {dlogits:.1f} x yardstick")
    assert max(score, dlogits) >= 2 * ht.MARGIN


@pytest.mark.parametrize("L", [17, 129])
def test_the_fault_the_device_had_is_rejected_under_head(L):
    """tf_score formed log_softmax as v - (log s + max): exact enough until the logits reach the tens, where the sum is rounded
    at their magnitude and a peaked row's 1 - softmax at the token, the whole of d logits there, loses half its value. The device
    sat at 4.5 x the bound of stage E's d logits under `head` (17 residues, 128 wide) until the kernel subtracted the maximum first."""
    e = hr.PEAKED["head"]
    score, dlogits = (d / y for y, d, _ in hr.stage_e_distances(L, PLUS_MAX, "head", e))
    print(f"[mutant] lse_plus_max under head 2^{e}, L = {L}: score {score:.1f}, d logits {dlogits:.1f} x yardstick")
    assert dlogits >= 2 * ht.MARGIN


@pytest.mark.parametrize("L", [129, 237])
def test_an_accumulator_not_rescaled_at_a_rising_maximum_is_rejected_under_sharp(L):
    e = hr.PEAKED["sharp"]
    b, bw = _worst("B", L, NO_RESCALE, "sharp", e), min(d / y for y, d, _ in hr.backward_distances(L, NO_RESCALE, "sharp", e))
    print(f"[mutant] online_no_rescale under sharp 2^{e}, L = {L}: stage B {b:.0f}, backward {bw:.0f} x yardstick")
    assert b >= 2 * ht.MARGIN and bw >= 2 * ht.MARGIN

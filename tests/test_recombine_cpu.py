"""Recombination without a GPU: the pairing, the cut, the exact pair matrix and its planted faults (tests/helpers_recombine.py),
and ppde_amd/recombine.py's summary and lineage on a hand-written record set."""
import functools

import numpy as np
import pytest

import helpers_library as hl
import helpers_recombine as hrc
import helpers_reversible as hr
import helpers_tempering as ht
from ppde_amd import recombine as rcb

DB_BOUND = 5e-6                  # tests/test_reversible_cpu.py's bound on the relative detailed-balance residual
POWER_START_A, POWER_START_C = hrc.POWER_START_A, hrc.POWER_START_C


@pytest.mark.parametrize("D", [2, 4, 6, 10])
def test_partners_is_a_round_robin(D):
    met = set()
    for s in range(D - 1):
        p = hrc.partners(s, D)
        assert sorted(p) == list(range(D)) and (p != np.arange(D)).all() and np.array_equal(p[p], np.arange(D))
        met |= {(min(i, int(p[i])), max(i, int(p[i]))) for i in range(D)}
        assert np.array_equal(hrc.partners(s + D - 1, D), p)
    assert len(met) == D * (D - 1) // 2                                      # every pair exactly once: (D - 1) D / 2 meetings


def test_the_cut_is_ordered_and_in_range():
    for S_o in (1, 2, 3, 16, 237):
        lo, hi, u = hrc.cut(99, np.arange(4000), 5, S_o)
        assert (0 <= lo).all() and (lo <= hi).all() and (hi < S_o).all() and (0 <= u).all() and (u < 1).all() and u.dtype == np.float32
        if S_o > 1:
            assert (lo < hi).any() and (lo == hi).any()
        p = hrc.cut_probabilities(S_o)
        assert abs(sum(p.values()) - 1.0) < 1e-12
        if S_o == 16:                                                        # a power of two: mulhi is exactly uniform
            assert p[(3, 3)] == 1 / 256 and p[(2, 9)] == 2 / 256
    lo2, hi2, u2 = hrc.cut(99, np.arange(4000), 6, 16)
    assert not np.array_equal(u2, hrc.cut(99, np.arange(4000), 5, 16)[2])


def test_the_exchange_is_its_own_inverse():
    rng = np.random.default_rng(1)
    xa, xb = rng.integers(0, 20, 30), rng.integers(0, 20, 30)
    sites = np.array([3, 4, 9, 20])
    ca, cb = hrc.cross(xa, xb, sites)
    ba, bb = hrc.cross(ca, cb, sites)
    assert np.array_equal(ba, xa) and np.array_equal(bb, xb)
    keep = np.setdiff1d(np.arange(30), sites)
    assert np.array_equal(ca[keep], xa[keep]) and np.array_equal(ca[sites], xb[sites])


@functools.lru_cache(maxsize=None)
def _case(name, nmut):
    c = dict(ht.case_a(), nmut=nmut) if name == "A" else hrc.case_c()
    en = hl.oracle_energy_of(c)
    K, states, index, E, inside = hr.exact_reversible_kernel(en, c["wt"], c["allowed"], 2, 0, c["L"] - 1, nmut)
    e32, _ = en.energy(states)
    positions = np.flatnonzero(c["allowed"])
    return c, K, states.numpy(), index, E, inside, e32.numpy(), positions


def _matrix(name, nmut, fault=None):
    c, K, states, index, E, inside, e32, positions = _case(name, nmut)
    return hrc.pair_matrix(states, positions, e32, inside, fault)


def _residual_inside(X, pi2):
    live = pi2 > 0
    return hr.detailed_balance_residual(X[np.ix_(live, live)], pi2[live])


@pytest.mark.parametrize("nmut", [0, 2])
def test_the_pair_matrix_keeps_the_product_law(nmut):
    """Case A: 35 states, two open residues, 1225 joint states (11 states under the cap with nmut = 2)."""
    c, K, states, index, E, inside, e32, positions = _case("A", nmut)
    assert states.shape[0] == 35 and len(positions) == 2 and int(inside.sum()) == (35 if nmut == 0 else 11)
    X = _matrix("A", nmut)
    pi = hr.target_law(E, inside)
    pi2 = np.kron(pi, pi)
    live = pi2 > 0
    assert np.abs(X.sum(1) - 1.0).max() < 1e-12 and (X >= 0).all()
    assert np.abs(pi2 @ X - pi2).max() <= DB_BOUND * pi2.max()
    res = _residual_inside(X, pi2)
    print(f"recombination pair matrix nmut={nmut}: detailed-balance residual {res:.3g}")
    assert res <= DB_BOUND
    assert X[np.ix_(live, ~live)].sum() == 0.0                               # no pair ever leaves the cap
    if nmut == 2:                                                            # two single mutants at different residues: a child at the cap
        wt_letters = [int(c["wt"][p]) for p in positions]
        a = next(i for i in np.flatnonzero(inside) if states[i, positions[0]] != wt_letters[0])
        b = next(i for i in np.flatnonzero(inside) if states[i, positions[1]] != wt_letters[1])
        S = states.shape[0]
        # a one-residue segment makes a double mutant (rejected, probability 1/2 in all); the whole-row exchange only swaps the two
        assert X[a * S + b, a * S + b] == 0.5 and X[a * S + b, b * S + a] == 0.5


@pytest.mark.parametrize("fault,nmut", [("ratio_a", 0), ("write_a", 0), ("cap_one", 2)])
def test_the_pair_matrix_rejects_the_planted_faults(fault, nmut):
    c, K, states, index, E, inside, e32, positions = _case("A", nmut)
    X = _matrix("A", nmut, fault)
    pi = hr.target_law(E, inside)
    pi2 = np.kron(pi, pi)
    moved = np.abs(pi2 @ X - pi2).max() / pi2.max()
    print(f"planted fault {fault}: stationary law moves by {moved:.3g} of its largest cell")
    assert moved > 100 * DB_BOUND


def test_the_pairing_fault_changes_the_law_of_a_deme_of_four():
    c, K, states, index, E, inside, e32, positions = _case("C", 0)
    assert states.shape[0] == 8 and len(positions) == 3
    X = _matrix("C", 0)
    pi = hr.target_law(E, inside)
    pi2 = np.kron(pi, pi)
    assert np.abs(X.sum(1) - 1.0).max() < 1e-12 and _residual_inside(X, pi2) <= DB_BOUND
    pi4 = np.kron(pi2, pi2)
    for s in range(3):                                                       # every round keeps the product law of the deme
        assert np.abs(hrc.apply_event(pi4, X, s, 4, 8) - pi4).max() <= DB_BOUND * pi4.max()
    j0 = int(np.ravel_multi_index(POWER_START_C, (8,) * 4))
    good = hrc.joint_law_recombined(3, K, X, 1, 4, j0)
    bad = hrc.joint_law_recombined(3, K, X, 1, 4, j0, fault="round0")
    assert abs(good.sum() - 1.0) < 1e-12 and hr.total_variation(good, bad) > 1e-3


def _power(name, nmut, D, n_demes, start, fault):
    """The largest expected Pearson statistic over the GPU law tests' (T, every) of a sample from the faulty law, over its bound."""
    c, K, states, index, E, inside, e32, positions = _case(name, nmut)
    S = states.shape[0]
    X, Xf = _matrix(name, nmut), (_matrix(name, nmut) if fault == "round0" else _matrix(name, nmut, fault))
    j0 = int(np.ravel_multi_index(start, (S,) * D))
    best = 0.0
    for T in hrc.LAW_T:
        for every in hrc.LAW_EVERY:
            if T < every:
                continue
            good = hrc.joint_law_recombined(T, K, X, every, D, j0)
            bad = hrc.joint_law_recombined(T, K, Xf, every, D, j0, fault="round0" if fault == "round0" else None)
            stat, df = ht.expected_pearson(good, bad, n_demes)
            best = max(best, stat / hl.chi_square_bound(df))
    return best


@pytest.mark.parametrize("name,nmut,D,n_demes,fault", [("A", 0, 2, 1 << 16, "ratio_a"), ("A", 0, 2, 1 << 16, "write_a"),
                                                      ("A", 2, 2, 1 << 16, "cap_one"), ("C", 0, 4, 1 << 15, "round0")])
def test_the_law_tests_can_see_every_fault(name, nmut, D, n_demes, fault):
    """At the GPU law tests' sample sizes and start states the expected Pearson statistic of a run with the fault exceeds
    helpers_library.chi_square_bound in at least one of their (T, every). The start states were picked by evaluating _power over
    candidate joint states and keeping one that every applicable fault clears with room."""
    start = POWER_START_A[nmut] if name == "A" else POWER_START_C
    ratio = _power(name, nmut, D, n_demes, start, fault)
    print(f"power against {fault} from {start}: expected statistic / bound = {ratio:.2f}")
    assert ratio > 1.0


# ------------------------------------------------------------------------------------------------ summary and lineage
def _records():
    """Two events of 4 chains, open sites (2, 3, 5, 7). Event 0 pairs (0, 3), (1, 2); event 1 pairs (0, 1), (2, 3)."""
    z = np.zeros((2, 4))
    return dict(partner=np.array([[3, 2, 1, 0], [1, 0, 3, 2]]), lo=np.array([[1, 0, 0, 1], [2, 2, 3, 3]]),
                hi=np.array([[2, 0, 0, 2], [3, 3, 3, 3]]), differ=np.array([[2, 0, 0, 2], [1, 1, 1, 1]]),
                outcome=np.array([[1, 1, 1, 1], [0, 0, 2, 2]], np.uint8), child_dist=z, log_ratio=z, pre_energy=z, child_energy=z)


def test_summarise_on_a_hand_written_record_set():
    s = rcb.summarise(_records())
    assert s["pairs"] == 4 and s["identical_share"] == 0.25 and s["capped_share"] == 0.25 and s["not_finite_share"] == 0.0
    assert s["acceptance"] == pytest.approx(1 / 3)                           # of the three pairs with differ > 0 one was accepted
    assert s["by_length"] == {2: (2, 0.5), 1: (1, 0.0)} and s["by_differ"] == {2: (1, 1.0), 1: (2, 0.0)}
    assert rcb.summarise({k: v[:0] for k, v in _records().items()})["pairs"] == 0


def test_lineage_on_a_hand_written_record_set():
    who = rcb.lineage(_records(), [2, 3, 5, 7], 4, 8)
    want = np.tile(np.arange(4)[:, None], (1, 8))
    want[0, [3, 5]], want[3, [3, 5]] = 3, 0                                  # event 0, pair (0, 3): open[1..2] = residues 3, 5
    want[1, 2], want[2, 2] = 2, 1                                            # pair (1, 2): open[0..0] = residue 2 (identical letters, still exchanged)
    assert np.array_equal(who, want)                                         # event 1: nothing accepted
    rec = _records()
    rec["outcome"][1] = 1
    who = rcb.lineage(rec, [2, 3, 5, 7], 4, 8)
    want[0, [5, 7]], want[1, [5, 7]] = want[1, [5, 7]].copy(), want[0, [5, 7]].copy()
    want[2, 7], want[3, 7] = want[3, 7], want[2, 7]
    assert np.array_equal(who, want) and who[1, 5] == 3                      # residue 5 of chain 1 descends from chain 3 through chain 0


def test_host_side_under_address_sanitizer():
    """tests/hostcheck/recombine.cpp: the refusals, set / replace / clear, the reads, an event-aligned and a misaligned run sequence
    and the failure sweep over every fallible runtime call, against the mock runtime under ASan + LSan."""
    import os
    import re
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "recombine", "sweep"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck recombine ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

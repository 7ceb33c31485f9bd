"""Forbidden patterns without a GPU: the text form, `find` against the definition, the active words, the CPU iteration of the mode,
the exact constrained kernel on the law case, and the planted faults (tests/helpers_motifs.py)."""
import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_motifs as hm
import helpers_reversible as hr
from ppde_amd import motifs
from ppde_amd.encoding import ALPHABET

A = 20
bit = lambda s: sum(1 << ALPHABET.index(ch) for ch in s)


# ------------------------------------------------------------------------------------------------ the text form
def test_parse_reads_letters_sets_complements_any_and_repetitions():
    pt = motifs.parse("N{P}[ST], NG, K(4), x(2)C")
    assert len(pt) == 4 and pt.lengths.tolist() == [3, 2, 4, 3]
    assert pt.elements[0, :4].tolist() == [bit("N"), motifs.ALL_LETTERS & ~bit("P"), bit("ST"), 0]
    assert pt.elements[1, :3].tolist() == [bit("N"), bit("G"), 0]
    assert pt.elements[2, :5].tolist() == [bit("K")] * 4 + [0]
    assert pt.elements[3, :3].tolist() == [motifs.ALL_LETTERS, motifs.ALL_LETTERS, bit("C")]
    assert pt.text == ["N{P}[ST]", "NG", "K(4)", "x(2)C"]
    again = motifs.parse(["N{P}[ST]", "NG", "K(4)", "x(2)C"])
    assert np.array_equal(again.elements, pt.elements) and np.array_equal(again.lengths, pt.lengths)
    assert motifs.element_text(pt.elements[0], 3) == "N[ACDEFGHIKLMNQRSTVWY][ST]"
    assert motifs.parse(pt) is pt


def test_presets():
    assert motifs.PRESETS == {"n_glycosylation": "N{P}[ST]", "deamidation": "N[GS]", "isomerisation": "D[GS]"}
    pt = motifs.parse("n_glycosylation, deamidation,isomerisation")
    assert pt.text == ["N{P}[ST]", "N[GS]", "D[GS]"] and pt.lengths.tolist() == [3, 2, 2]
    assert pt.elements[2, :2].tolist() == [bit("D"), bit("GS")]


@pytest.mark.parametrize("text, column, what", [
    ("NB", 1, "not one of"), ("N[ST", 1, "never closed"), ("N{P", 1, "never closed"), ("N[]", 1, "holds no letter"),
    ("{ACDEFGHIKLMNPQRSTVWY}", 0, "holds no letter"), ("(3)N", 0, "repetition"), ("N(0)", 1, "repetition"), ("N(a)", 1, "repetition"),
    ("N(2", 1, "repetition"), ("K(9)", 1, "more than 8"), ("ACDEFGHIK", 8, "more than 8"), ("N[SZ]", 3, "not one of"), ("n", 0, "not one of"),
])
def test_parse_refusals_name_the_pattern_and_the_column(text, column, what):
    with pytest.raises(ValueError, match=what) as e:
        motifs.parse("NG," + text)
    assert repr(text) in str(e.value) and f"column {column}" in str(e.value)


def test_parse_refuses_nothing_and_too_much():
    with pytest.raises(ValueError, match="no pattern"):
        motifs.parse("")
    with pytest.raises(ValueError, match="empty pattern"):
        motifs.parse("NG,,DG")
    with pytest.raises(ValueError, match="at most 32"):
        motifs.parse(["NG"] * 33)
    assert len(motifs.parse(["NG"] * 32)) == 32


def test_check_patterns_makes_the_setters_checks():
    with pytest.raises(ValueError, match="exceeds the sequence length"):
        motifs.check_patterns("K(5)", 4)
    with pytest.raises(ValueError, match="empty set or a bit"):
        motifs.check_patterns(motifs.Patterns(np.array([[1 << 20, 0, 0, 0, 0, 0, 0, 0]]), [1]), 9)
    with pytest.raises(ValueError, match="empty set or a bit"):
        motifs.check_patterns(motifs.Patterns(np.array([[1, 0, 0, 0, 0, 0, 0, 0]]), [2]), 9)
    with pytest.raises(ValueError, match="length must be in"):
        motifs.check_patterns(motifs.Patterns(np.ones((1, 8)), [9]), 12)
    assert len(motifs.check_patterns("K(4)", 4)) == 1


# ------------------------------------------------------------------------------------------------ find
@pytest.mark.parametrize("L", [1, 7, 8, 24, 65])
def test_find_against_the_definition_on_random_rows(L):
    rng = np.random.default_rng(100 + L)
    pt = hm.random_patterns(rng, 32, density=0.5)
    idx = rng.integers(0, A, (200, L)).astype(np.uint8)
    wt = rng.integers(0, A, L).astype(np.uint8)
    for allow in (True, False):
        act = motifs.active_mask(pt, L, wt, allow)
        got = motifs.find(idx, pt, wt, allow)
        want = hm.brute_find(idx, pt, act)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    free = motifs.find(idx, pt)[0] < 0
    assert np.array_equal(free, motifs.is_free(idx, pt))


def test_find_at_the_edges():
    L = 12
    pt = motifs.Patterns(np.vstack([np.r_[[bit("C")] * 8], np.zeros((30, 8)) + bit("W"), np.r_[bit("N"), bit("G"), [0] * 6]]),
                         [8] + [3] * 30 + [2])
    row = np.full(L, ALPHABET.index("A"), np.uint8)
    at = lambda r: tuple(int(v[0]) for v in motifs.find(r[None], pt))
    assert at(row) == (-1, -1)
    r = row.copy(); r[0:2] = [ALPHABET.index("N"), ALPHABET.index("G")]
    assert at(r) == (31, 0)                                  # pattern index 31, a window at p = 0
    r = row.copy(); r[L - 2:] = [ALPHABET.index("N"), ALPHABET.index("G")]
    assert at(r) == (31, L - 2)                              # a window at p = L - len
    r = row.copy(); r[L - 8:] = ALPHABET.index("C")
    assert at(r) == (0, L - 8)                               # len = 8 at the last start
    r[L - 8] = ALPHABET.index("A")
    assert at(r) == (-1, -1)
    r = row.copy(); r[:] = ALPHABET.index("C"); r[3:5] = [ALPHABET.index("N"), ALPHABET.index("G")]
    assert at(r) == (31, 3)                                  # C(8) does not fit around the NG: the higher pattern is the first
    r = row.copy(); r[:8] = ALPHABET.index("C"); r[9:11] = [ALPHABET.index("N"), ALPHABET.index("G")]
    assert at(r) == (0, 0)                                   # the lowest pattern wins, not the lowest position
    short = np.full((1, 5), ALPHABET.index("C"), np.uint8)   # len > L: the pattern has no window
    assert tuple(int(v[0]) for v in motifs.find(short, pt)) == (-1, -1)
    assert not motifs.active_mask(pt, 5)[0].any() and motifs.active_mask(pt, 5)[31, :4].all() and not motifs.active_mask(pt, 5)[31, 4]


def test_active_words_with_and_without_the_native_exemption():
    seq = "ANGSANGTAAN"                                       # the wild type matches NG at 1 and 5; a trailing N matches nothing
    wt = np.array([ALPHABET.index(ch) for ch in seq], np.uint8)
    L = len(seq)
    pt = motifs.parse("NG, N{P}[ST]")
    w1 = motifs.active_words(pt, L, wt, True)
    w0 = motifs.active_words(pt, L, wt, False)
    assert w1.dtype == np.uint32 and w0.dtype == np.uint32
    assert [int(v) & 1 for v in w0] == [1] * (L - 1) + [0]                                  # NG everywhere it fits
    assert [int(v) >> 1 for v in w0] == [1] * (L - 2) + [0, 0]
    assert [int(v) & 1 for v in w1] == [0 if p in (1, 5) else 1 for p in range(L - 1)] + [0]   # exempt per (pattern, position)
    assert [int(v) >> 1 for v in w1] == [0 if p in (1, 5) else 1 for p in range(L - 2)] + [0, 0]   # NGS / NGT are native sequons
    assert np.array_equal(motifs.active_words(pt, L), w0)                                   # no wild type: nothing exempt
    # whatever the chain puts at a native site later is no new liability; the same pattern elsewhere is
    x = wt.copy(); x[7] = ALPHABET.index("S")
    assert motifs.find(x[None], pt, wt, True)[0][0] == -1 and motifs.find(x[None], pt, wt, False)[0][0] == 0
    y = wt.copy(); y[8:10] = [ALPHABET.index("N"), ALPHABET.index("G")]
    assert tuple(int(v[0]) for v in motifs.find(y[None], pt, wt, True)) == (0, 8)


def test_summarise_and_the_log_line():
    v = np.zeros((4, 2), np.int64); v[:, 0] = [5, 5, 5, 5]; v[:, 1] = [1, 2, 3, 4]
    s = motifs.summarise(v, 50, ["N{P}[ST]", "NG"])
    assert s["per_pattern"].tolist() == [0.1, 0.05] and abs(s["share"] - 0.15) < 1e-12
    assert motifs.log_line(s) == "# forbidden patterns: vetoed 0.150 of the proposals so far (N{P}[ST]: 0.100, NG: 0.050)"


# ------------------------------------------------------------------------------------------------ the law case
@pytest.fixture(scope="module")
def law():
    c = hr.cap_case()
    assert c["wt"].tolist() == [1, 13, 16, 9, 17, 16, 18]
    pt = hm.law_patterns(c)
    en = hl.oracle_energy_of(c)
    out = {}
    for nmut in (0, 2):
        K, states, index, e, inside = hr.exact_reversible_kernel(en, c["wt"], c["allowed"], 2, 0, c["L"] - 1, nmut)
        free = motifs.is_free(states.numpy(), pt, c["wt"], True)
        out[nmut] = (K, states, index, e, inside, free)
    return c, pt, en, out


def test_the_exact_constrained_kernel(law):
    c, pt, _, out = law
    for nmut, n_free, df in ((0, 68, 67), (2, 16, 15)):
        K, states, index, e, inside, free = out[nmut]
        Kc, ins = hm.constrain_kernel(K, inside, free)
        assert int(ins.sum()) == n_free and int(inside.sum()) == (121 if nmut == 0 else 21)
        assert np.abs(Kc[ins].sum(1) - 1.0).max() <= 3e-16 and (Kc >= 0).all()
        assert Kc[np.ix_(ins, ~ins)].sum() == 0.0                                           # no flow leaves the free set
        pi = hr.target_law(e, ins)
        assert hr.detailed_balance_residual(Kc[np.ix_(ins, ins)], pi[ins]) <= 5e-6
        st = hr.stationary_vector(Kc[np.ix_(ins, ins)])
        assert hr.total_variation(st, pi[ins]) <= 2e-8
        wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
        assert ins[wt_row]
        for T in (1, 2, 3, 8):
            row = np.linalg.matrix_power(Kc, T)[wt_row]
            assert (row[ins] * (1 << 16) >= 8).all() and row[~ins].sum() == 0.0
            assert hl.chi_square(np.round(row * (1 << 16)), row * (1 << 16))[1] == df
        # what the constraint removes: the unconstrained kernel's mass on forbidden states at T = 8
        lost = np.linalg.matrix_power(K, 8)[wt_row][inside & ~free].sum()
        assert abs(lost - (0.35 if nmut == 0 else 0.15)) < 0.01


def test_the_cpu_iteration_samples_the_constrained_kernel(law):
    """4096 chains, one iteration from the wild type on torch's noise: the chi-square of the CPU iteration against the row of the
    exact constrained kernel; vetoes are counted by lowest pattern and no chain sits on a forbidden state."""
    c, pt, en, out = law
    K, states, index, e, inside, free = out[0]
    Kc, ins = hm.constrain_kernel(K, inside, free)
    n = 4096
    gen = torch.Generator().manual_seed(5)
    import ppde_oracle as orc
    noise = [orc.draw_noise_torch(n, c["L"] * A, 2, generator=gen) for _ in range(2)]
    res = hm.constrained_run(en, np.tile(c["wt"].astype(np.int64), (n, 1)), c["wt"], lambda t: noise[t], 2, 0, c["L"] - 1, 2, 0, c["allowed"], pt)
    cells, bad = hl.state_cells(res["final_idx"].numpy(), c["allowed"], index, c["wt"])
    assert bad == 0 and ins[cells].all()
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    chi2, df = hl.chi_square(np.bincount(cells, minlength=len(ins)).astype(np.float64), n * np.linalg.matrix_power(Kc, 2)[wt_row])
    assert df >= 10 and chi2 < hl.chi_square_bound(df)
    props = np.stack([t["proposal"].numpy() for t in res["traces"]])
    fp = np.stack([motifs.find(p, pt, c["wt"])[0] for p in props])
    want = np.stack([(fp == m).sum(0) for m in range(len(pt))], 1)
    assert np.array_equal(res["vetoes"], want) and (want.sum(0) > 0).all()
    acc = res["accepted"].numpy()
    assert not acc[fp >= 0].any() and acc.any()
    e_hist = res["energy_history"].numpy()
    assert np.array_equal(e_hist[1:][fp >= 0], e_hist[:-1][fp >= 0])                        # a veto records the current energy


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("name", hm.REPLAY_NAMES)
def test_replay_cases_veto_a_tenth_and_keep_their_distance_from_ties(name, rng_mode):
    """On the reference alone, as tests/test_reversible_cpu.py does for the runs without patterns."""
    c, lib = hr.replay_model()
    noise, ref, pt = hm.replay_reference(name, rng_mode, hl.oracle_energy_of(c), c, lib, keep_probs=True)
    assert hm.veto_share(ref) >= 0.1 and (ref["vetoes"].sum(0)[:2] > 0).all()
    decided = [dict(o, refused=o["refused"] | o["veto"]) for o in ref["traces"]]           # the decisions u takes
    acc_margin, gap = hr.replay_margins(noise, dict(ref, traces=decided))
    print(f"{name} rng_mode {rng_mode}: vetoed {hm.veto_share(ref):.3f}, smallest |log_acc - log u| {acc_margin:.3g}, race gap {gap:.3g}")
    assert acc_margin > 2e-3 and gap > 1e-4
    veto = torch.stack([o["veto"] for o in ref["traces"]])
    assert ref["accepted"].any() and not (veto & ref["accepted"]).any()
    assert motifs.is_free(ref["states"].reshape(-1, c["L"]).numpy(), pt, c["wt"]).all()


# ------------------------------------------------------------------------------------------------ planted faults
def _law_shift(law, act_fault, nmut=0, T=8):
    """chi-square at 2^16 chains of the expected counts of a kernel built with a faulty free set against the true one's"""
    c, pt, _, out = law
    K, states, index, e, inside, free = out[nmut]
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    free_f = hm.find_with(states.numpy(), pt, act_fault)[0] < 0
    good = np.linalg.matrix_power(hm.constrain_kernel(K, inside, free)[0], T)[wt_row] * (1 << 16)
    bad = np.linalg.matrix_power(hm.constrain_kernel(K, inside, free_f)[0], T)[wt_row] * (1 << 16)
    return hl.chi_square(bad, good), int((free_f != free)[inside].sum())


def test_fault_last_start_skipped_breaks_find_parity():
    rng = np.random.default_rng(3)
    pt = motifs.parse("NG, K(4)")
    L = 9
    row = hm.plant(np.full(L, ALPHABET.index("A"), np.uint8), pt, 1, L - 4, rng)
    act = hm.faulty_active(pt, L, None, True, "last_start_skipped")
    assert motifs.find(row[None], pt)[0][0] == 1 and hm.find_with(row[None], pt, act)[0][0] == -1


def test_fault_frozen_residues_not_context_moves_the_law(law):
    c, pt, _, _ = law
    act = hm.faulty_active(pt, c["L"], c["wt"], True, "frozen_not_context", c["allowed"])
    assert act[0, 2] and not act[1, 1] and not act[2, 3]                                    # P1 and P2 go unenforced at their sites
    for nmut in (0, 2):
        (chi2, df), moved = _law_shift(law, act, nmut)
        assert moved > 0 and chi2 > 10 * hl.chi_square_bound(df)


def test_fault_native_exemption_per_pattern_breaks_find_parity_and_moves_the_law(law):
    seq = "ANGAAAAAA"
    wt = np.array([ALPHABET.index(ch) for ch in seq], np.uint8)
    pt = motifs.parse("NG")
    x = wt.copy(); x[5:7] = [ALPHABET.index("N"), ALPHABET.index("G")]
    act = hm.faulty_active(pt, len(seq), wt, True, "native_per_pattern")
    assert motifs.find(x[None], pt, wt, True)[0][0] == 0 and hm.find_with(x[None], pt, act)[0][0] == -1
    # on the law case: a fourth pattern the wild type matches at residues 0-1 and that also covers P0's states
    c, pt3, _, out = law
    el = np.vstack([pt3.elements, np.zeros((1, 8), np.uint32)])
    el[3, :2] = [(1 << int(c["wt"][0])) | int(pt3.elements[0, 0]), (1 << int(c["wt"][1])) | int(pt3.elements[0, 1])]
    pt4 = motifs.Patterns(el, [2, 2, 2, 2])
    states = out[0][1].numpy()
    rule = motifs.active_mask(pt4, c["L"], c["wt"], True)
    fault = hm.faulty_active(pt4, c["L"], c["wt"], True, "native_per_pattern")
    assert not rule[3, 0] and rule[3, 2] and not fault[3].any()
    assert np.array_equal(motifs.is_free(states, pt4, c["wt"]), motifs.is_free(states, pt3, c["wt"]))   # P3 adds nothing to P0 here ...
    assert np.array_equal(hm.find_with(states, pt4, fault)[0] < 0, motifs.is_free(states, pt3, c["wt"]))  # ... so the law needs `find`


def test_fault_veto_through_u_accepts_at_u_zero(law):
    c, pt, en, _ = law
    n = 256
    gen = torch.Generator().manual_seed(11)
    import ppde_oracle as orc
    U, q, u = orc.draw_noise_torch(n, c["L"] * A, 2, generator=gen)
    u = torch.zeros_like(u)
    wt = torch.as_tensor(c["wt"].astype(np.int64))
    cur = wt.repeat(n, 1)
    thr = hr._threshold(0)
    good = hm.constrained_iteration(en, cur, wt, U, q, u, 0, c["L"] - 1, thr, c["allowed"], pt)
    bad = hm.constrained_iteration(en, cur, wt, U, q, u, 0, c["L"] - 1, thr, c["allowed"], pt, fault="veto_through_u")
    v = good["veto"].numpy()
    assert v.any() and not good["accepted"].numpy()[v].any()
    assert bad["accepted"].numpy()[v & ~good["refused"].numpy()].all()                      # expf(-inf) = 0 >= u = 0
    assert not motifs.is_free(bad["idx"].numpy(), pt, c["wt"]).all()


def test_fault_one_child_only_lets_a_forbidden_child_in(law):
    """The child check of recombination: a pair is refused when EITHER child is not free."""
    c, pt, _, out = law
    states = out[0][1].numpy()
    free = out[0][5]
    # two free parents whose exchange of residue 3 gives one free and one forbidden child
    found = None
    for a in np.flatnonzero(free):
        for b in np.flatnonzero(free):
            ca, cb = states[a].copy(), states[b].copy()
            ca[3], cb[3] = states[b][3], states[a][3]
            fa, fb = motifs.is_free(np.stack([ca, cb]), pt, c["wt"])
            if fa and not fb:
                found = (ca, cb)
                break
        if found:
            break
    assert found is not None
    both = (motifs.find(np.stack(found), pt, c["wt"])[0] >= 0).any()
    first_only = motifs.find(found[0][None], pt, c["wt"])[0][0] >= 0
    assert both and not first_only

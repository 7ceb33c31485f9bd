"""Forbidden patterns on the GPU (ppde_chains_set_forbidden_patterns; k_motif_veto, k_motif_scan): the scan against
ppde_amd/motifs.py's `find`, patterns that never match change no bit, replays of the CPU iteration of the mode
(tests/helpers_motifs.py), graph replay / gradient policies / streams / sharding, the law against the exact constrained kernel,
the invariants across the other modes, the native exemption, the refusals, PPDE_PAS and the driver.

Everything discrete is compared exactly. Replays use tests/test_reversible_gpu.py's tolerances for the same quantities (log
acceptance ratios 2e-4, energy histories 2e-5, fitness 5e-6); the law uses tests/helpers_library.py's statistic and bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_motifs as hm
import helpers_recombine as hrc
import helpers_reversible as hr
from helpers import device_noise
from ppde_amd import library as dl
from ppde_amd import motifs
from ppde_amd.encoding import ALPHABET

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
PEEK_KEYS = ("idx", "energy", "fitness", "accepted", "dist")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, patterns=None, allow_native=True, x0=None, lo=None, hi=None, init=True,
            before_init=None, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", 99)
    lo = 0 if lo is None else lo
    hi = case["L"] - 1 if hi is None else hi
    ch = Chains(m, n, T, pas, nmut, False, lo, hi, 3 if case.get("cnn") is not None else 1, rng_mode, **kw)
    if lib is not None:
        ch.set_library(lib)
    ch.set_reversible(True)
    if patterns is not None:
        ch.set_forbidden(patterns, allow_native)
    if before_init is not None:
        before_init(ch)
    if init:
        ch.init(torch.as_tensor(np.tile(case["wt"], (n, 1)) if x0 is None else x0).cuda())
    return ch


def _noise(rng_mode, n, c, T, pas=2, seed=77):
    import ppde_oracle as orc
    if rng_mode != 0:
        return None
    gen = torch.Generator().manual_seed(seed)
    return [orc.draw_noise_torch(n, c["L"] * 20, pas, generator=gen) for _ in range(T)]


def _run(ch, T, noise=None, first=0):
    if noise is None:
        ch.run(T)
        return
    for U, q, u in noise[first:first + T]:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _same(a, b, keys, label=""):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def _proposals(peeks, tr):
    """[T, n, L]: the proposals of a stepped, traced run, rebuilt from the states in front of every iteration and the traced moves."""
    out = []
    for t in range(tr["U"].shape[0]):
        y = peeks[t]["idx"].copy()
        for s in range(tr["flat"].shape[1]):
            act = np.flatnonzero(s < tr["U"][t])
            y[act, tr["flat"][t, s, act] // 20] = tr["flat"][t, s, act] % 20
        out.append(y)
    return np.stack(out)


def _veto_counts(props, pt, wt, allow_native=True):
    fp = np.stack([motifs.find(p, pt, wt, allow_native)[0] for p in props])
    return np.stack([(fp == m).sum(0) for m in range(len(pt))], 1).astype(np.int64), fp


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, m, hl.oracle_energy_of(c)
    m.close()


# ------------------------------------------------------------------------------------------------ 1. the scan
@pytest.mark.parametrize("L", [7, 24, 63, 64, 65, 130, 256])
def test_scan_equals_find(L):
    """M = 32 with lengths 1..8, n in 1, 3, 130: random rows, rows with a match planted at p = 0 and at p = L - len, at every start
    57..64 (across the 64-lane seam), and of pattern 31 only; with and without the native exemption."""
    from ppde_amd.energy import HipModel
    rng = np.random.default_rng(900 + L)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    m = HipModel(wt, "cuda:0")
    top = min(8, L)                                          # (a pattern longer than the sequence is refused: L = 7 runs 1..7)
    dense = hm.random_patterns(rng, 32, 0.5, top)            # random rows match often
    sparse = hm.random_patterns(rng, 32, 0.12, top)          # rows near the wild type are mostly free: planted matches decide
    for mm in np.flatnonzero(sparse.lengths <= 2):           # ... and pattern 31, over the letters A and C alone, can be the only one
        for j in range(int(sparse.lengths[mm])):
            sparse.elements[mm, j] = (int(sparse.elements[mm, j]) & ~3) or 4
    sparse.elements[31, :int(sparse.lengths[31])] = 3
    assert dense.lengths.tolist() == [1 + k % top for k in range(32)] and set(dense.lengths.tolist()) == set(range(1, top + 1))
    seam = False
    for pt in (dense, sparse):
        fits = np.flatnonzero(pt.lengths <= L)
        for n in (1, 3, 130):
            rows = rng.integers(0, 20, (n, L)).astype(np.uint8)
            if pt is sparse:                                 # the wild type with up to two residues changed
                rows = np.tile(wt, (n, 1))
                for i in range(n):
                    for l in rng.integers(0, L, int(rng.integers(3))):
                        rows[i, l] = rng.integers(20)
            for i in range(n):
                kind = (i + n) % 5
                mm = int(rng.choice(fits))
                ln = int(pt.lengths[mm])
                if kind == 1:
                    rows[i] = hm.plant(rows[i], pt, mm, 0, rng)
                elif kind == 2:
                    rows[i] = hm.plant(rows[i], pt, mm, L - ln, rng)
                elif kind == 3 and L - ln >= 57:
                    rows[i] = hm.plant(rows[i], pt, mm, min(57 + i % 8, L - ln), rng)
                elif kind == 4:
                    rows[i] = hm.plant(rows[i], pt, 31, int(rng.integers(L - int(pt.lengths[31]) + 1)), rng)
            for allow in (True, False):
                fp, pos = motifs.scan(m, rows, pt, allow)
                want = motifs.find(rows, pt, wt, allow)
                assert np.array_equal(fp, want[0]) and np.array_equal(pos, want[1]), (L, n, allow)
                kept, keep = motifs.filter_free(m, rows, pt, allow)
                assert np.array_equal(keep, want[0] < 0) and np.array_equal(kept, rows[want[0] < 0])
                seam |= bool(((want[1] >= 57) & (want[1] <= 64)).any())
                if pt is sparse and n == 130 and allow:
                    assert (want[0] == 31).any() and (want[0] == -1).any()                  # pattern 31 alone decided a row
    assert seam or L < 63
    m.close()


# ------------------------------------------------------------------------------------------------ 2. patterns that never match
def _unreachable_patterns(c, lib):
    """Patterns no state of the run can match: runs k(j) of a letter k such that no window of j residues can hold k everywhere
    (a residue can hold its wild-type letter and, when open, its library's letters)."""
    reach = np.asarray(dl.as_words(lib, c["L"])) | (1 << c["wt"].astype(np.int64))
    out = []
    for k in range(20):
        can = (reach >> k) & 1
        for j in range(1, 9):
            if not any(can[p:p + j].all() for p in range(c["L"] - j + 1)):
                out.append(f"{ALPHABET[k]}({j})" if j > 1 else ALPHABET[k])
                break
    return out


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("nmut", [0, 3])
def test_patterns_that_never_match_change_no_bit(toy, rng_mode, nmut):
    c, lib, m, _ = toy
    pats = _unreachable_patterns(c, lib)
    assert len(pats) >= 4
    n, T, lo, hi = 16, 20, c["i0"], c["i0"] + c["Lp"] - 1
    noise = _noise(rng_mode, n, c, T)
    for reuse in (True, False):
        out = []
        for p in (None, pats):
            ch = _chains(m, c, n, T, 2, nmut, rng_mode, lib, p, lo=lo, hi=hi, trace=True, reuse_grad=reuse)
            _run(ch, T, noise)
            out.append((ch.collect(), ch.peek(), ch.trace()))
            if p is not None:
                st = ch.forbidden_state()
                assert st["vetoes"].shape == (n, len(pats)) and not st["vetoes"].any() and st["n_patterns"] == len(pats)
                assert np.array_equal(st["active"], motifs.active_words(pats, c["L"], c["wt"], True))
            ch.close()
        _same(out[0][0], out[1][0], RESULT_KEYS, f"reuse={reuse}")
        _same(out[0][1], out[1][1], PEEK_KEYS, f"reuse={reuse}")
        _same(out[0][2], out[1][2], TRACE_KEYS, f"reuse={reuse}")
        assert out[0][2]["accepted"].any()


# ------------------------------------------------------------------------------------------------ 3. replays
def _against_reference(tr, res, ref, noise, T):
    for t in range(T):
        U = noise[t][0].numpy()
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    ref_la = np.stack([o["log_acc"].numpy() for o in ref["traces"]])
    assert np.abs(tr["log_acc"] - ref_la).max() <= 2e-4
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.abs(res["fitness_history"] - ref["fitness_history"].numpy()).max() <= 5e-6
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy())


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("name", hm.REPLAY_NAMES)
def test_replay_of_the_cpu_iteration_of_the_mode(toy, name, rng_mode):
    """rng_mode 0 on the reference's noise, rng_mode 1 on the device RNG's own draws restated on the CPU, stepped with a peek in
    front of every iteration: draws, accept bits, states and best states exact, and the counters equal `find` applied to the
    proposals rebuilt from the peeks and the traced moves."""
    c, lib, m, en = toy
    k = hr.REPLAY_CASES[name]
    pt = motifs.parse(hm.REPLAY_PATTERNS)
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    T = k["T"] if rng_mode == 0 else k["T_dev"]
    ch = _chains(m, c, k["n"], T, k["pas"], k["nmut"], rng_mode, lib, pt, lo=lo, hi=hi, seed=k["philox_seed"], trace=True,
                 reuse_grad=False, use_graph=False)
    noise = hr.replay_noise(name, 0, c["L"]) if rng_mode == 0 else device_noise(ch, T, k["pas"])
    peeks = [ch.peek()]
    for t in range(T):
        _run(ch, 1, noise if rng_mode == 0 else None, t)
        peeks.append(ch.peek())
    tr, res, st = ch.trace(), ch.collect(), ch.forbidden_state()
    ch.close()
    _, ref, _ = hm.replay_reference(name, rng_mode, en, c, lib, noise=noise)
    assert hm.veto_share(ref) >= 0.1                          # on the reference itself
    _against_reference(tr, res, ref, noise, T)
    for t in range(T + 1):
        assert np.array_equal(peeks[t]["idx"], ref["states"][t].numpy()), t
    props = _proposals(peeks, tr)
    assert np.array_equal(props, np.stack([o["proposal"].numpy() for o in ref["traces"]]))
    want, fp = _veto_counts(props, pt, c["wt"])
    assert np.array_equal(st["vetoes"], want) and np.array_equal(st["vetoes"], ref["vetoes"])
    assert (fp >= 0).any() and not tr["accepted"].astype(bool)[fp >= 0].any() and tr["accepted"].any()
    e = res["energy_history"]
    assert np.array_equal(e[1:][fp >= 0], e[:-1][fp >= 0])    # a veto records the current energy
    # the other gradient policy (the fused kernel on the device RNG) gives the same bits
    ch2 = _chains(m, c, k["n"], T, k["pas"], k["nmut"], rng_mode, lib, pt, lo=lo, hi=hi, seed=k["philox_seed"], trace=True, reuse_grad=True)
    _run(ch2, T, noise if rng_mode == 0 else None)
    _same(res, ch2.collect(), RESULT_KEYS, "reuse")
    _same(tr, ch2.trace(), TRACE_KEYS, "reuse")
    assert np.array_equal(ch2.forbidden_state()["vetoes"], st["vetoes"])
    ch2.close()


# ------------------------------------------------------------------------------------------------ 4. graphs, policies, streams, shards
@pytest.mark.parametrize("T", [120, 20, 7])
def test_graph_replay_equals_the_stepped_twin(toy, T):
    c, lib, m, _ = toy
    n, lo, hi = 16, c["i0"], c["i0"] + c["Lp"] - 1
    pt = hm.REPLAY_PATTERNS
    out = {}
    for label, kw, stepped in (("graph", dict(use_graph=True), False), ("stepped", dict(use_graph=False), True),
                               ("reeval", dict(use_graph=True, reuse_grad=False), False), ("streams", dict(n_streams=2), False)):
        ch = _chains(m, c, n, T, 2, 3, 1, lib, pt, lo=lo, hi=hi, **kw)
        if stepped:
            for _ in range(T):
                ch.run(1)
        else:
            ch.run(T)
        out[label] = (ch.collect(), ch.peek(), ch.forbidden_state()["vetoes"], ch.graph_stats())
        ch.close()
    assert out["graph"][3]["replayed_steps"] == (T if T >= 20 else 0) and out["stepped"][3]["replayed_steps"] == 0
    for label in ("stepped", "reeval", "streams"):
        _same(out["graph"][0], out[label][0], RESULT_KEYS, label)
        _same(out["graph"][1], out[label][1], PEEK_KEYS, label)
        assert np.array_equal(out["graph"][2], out[label][2]), label
    assert out["graph"][2].sum() >= 0.1 * n * T
    if T == 20:                                               # sharding by chain_offset changes nothing
        parts = []
        for n_, off in ((7, 0), (9, 7)):
            ch = _chains(m, c, n_, T, 2, 3, 1, lib, pt, lo=lo, hi=hi, chain_offset=off, random_chain=0 if off == 0 else -1)
            ch.run(T)
            parts.append((ch.collect(), ch.forbidden_state()["vetoes"]))
            ch.close()
        one = out["graph"]
        for k_ in ("energy_history", "fitness_history"):
            assert np.array_equal(np.concatenate([parts[0][0][k_], parts[1][0][k_]], 1), one[0][k_]), k_
        for k_ in ("best_idx", "best_energy", "best_step"):
            assert np.array_equal(np.concatenate([parts[0][0][k_], parts[1][0][k_]], 0), one[0][k_]), k_
        assert np.array_equal(np.concatenate([parts[0][1], parts[1][1]], 0), one[2])


# ------------------------------------------------------------------------------------------------ 5. the law
_LAW = {}


def _law(nmut):
    if nmut not in _LAW:
        c = hr.cap_case()
        pt = hm.law_patterns(c)
        K, states, index, e, inside = hr.exact_reversible_kernel(hl.oracle_energy_of(c), c["wt"], c["allowed"], 2, 0, c["L"] - 1, nmut)
        free = motifs.is_free(states.numpy(), pt, c["wt"], True)
        Kc, ins = hm.constrain_kernel(K, inside, free)
        _LAW[nmut] = (c, pt, Kc, states, index, ins)
    return _LAW[nmut]


@pytest.mark.parametrize("nmut", [0, 2])
def test_law_of_the_constrained_chains(nmut):
    """2^16 chains from the wild type after T = 1, 2, 3, 8 iterations against the matrix power of the exact constrained kernel;
    no chain on a forbidden state."""
    c, pt, Kc, states, index, ins = _law(nmut)
    assert int(ins.sum()) == (68 if nmut == 0 else 16)
    m = hl.hip_model_of(c)
    n = 1 << 16
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    for T in (1, 2, 3, 8):
        ch = _chains(m, c, n, T, 2, nmut, 1, c["allowed"], pt, random_chain=-1, seed=1977 + 13 * T + nmut)
        ch.run(T)
        idx = ch.peek()["idx"]
        ch.close()
        cells, bad = hl.state_cells(idx, c["allowed"], index, c["wt"])
        assert bad == 0 and ins[cells].all() and motifs.is_free(idx, pt, c["wt"]).all()
        chi2, df = hl.chi_square(np.bincount(cells, minlength=len(ins)).astype(np.float64), n * np.linalg.matrix_power(Kc, T)[wt_row])
        print(f"constrained law, nmut {nmut}, T={T}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
        assert df >= 10 and df == (67 if nmut == 0 else 15)
        assert chi2 < hl.chi_square_bound(df), (nmut, T, chi2, df)
    m.close()


# ------------------------------------------------------------------------------------------------ 6. the other modes
def _all_free(rows, pt, wt, label):
    rows = np.asarray(rows).reshape(-1, len(wt))
    assert motifs.is_free(rows, pt, wt).all(), label


def _observed_run(toy, before_init, T=24, n=16, x0=None, seed=99, patterns=hm.REPLAY_PATTERNS, nmut=3):
    c, lib, m, _ = toy
    pt = motifs.parse(patterns)

    def setup(ch):
        before_init(ch)
        ch.set_recorder(2)
        ch.set_archive(4)

    ch = _chains(m, c, n, T, 2, nmut, 1, lib, pt, lo=c["i0"], hi=c["i0"] + c["Lp"] - 1, x0=x0, before_init=setup, use_graph=False, seed=seed)
    peeks = [ch.peek()]
    for _ in range(T):
        ch.run(1)
        peeks.append(ch.peek())
    res, rec, arc, st = ch.collect(), ch.recorded(), ch.archive(), ch.forbidden_state()
    for t, p in enumerate(peeks):
        _all_free(p["idx"], pt, c["wt"], ("peek", t))
    _all_free(res["best_idx"], pt, c["wt"], "best")
    _all_free(rec["idx"], pt, c["wt"], "recorded")
    assert rec["rows"] == T // 2
    for b in range(n):
        if arc["count"][b]:
            _all_free(arc["idx"][b, :arc["count"][b]], pt, c["wt"], ("archive", b))
    assert arc["count"].any() and st["vetoes"].sum() > 0
    return ch, peeks, st, pt


def test_invariants_under_tempering(toy):
    ch, peeks, _, _ = _observed_run(toy, lambda ch: ch.set_tempering([1.0, 0.5], 1))
    assert ch.tempering_state()["swap_attempts"].sum() > 0
    ch.close()


def test_invariants_under_annealing(toy):
    ch, peeks, _, _ = _observed_run(toy, lambda ch: ch.set_annealing([0.25, 0.5, 0.75, 1.0], every=6, deme=8))
    assert ch.annealing_shape()[2] >= 1
    ch.close()


def test_invariants_under_recombination_and_outcome_4(toy):
    """every 2, deme 4, scattered free starts: outcome 4 exactly where a child is not free and outcomes 3 and 2 do not apply; the
    records of every pair obey the rules they obey without the mode. Two patterns over neighbouring letter classes and starts with
    4 or more residues changed, no cap: a child that joins two free parents' segments then matches often enough to be seen (a
    tenth of the pairs of the start population, counted with the rule alone)."""
    c, lib, m, _ = toy
    pats = "[ACDEFGH][IKLMNPQ], [RSTVWY]x[ACDEFGH]"
    pt = motifs.parse(pats)
    n, T, every, D, seed, lo, hi, nmut = 16, 24, 2, 4, 99, c["i0"], c["i0"] + c["Lp"] - 1, 0
    rng = np.random.default_rng(5)
    words = dl.as_words(lib, c["L"])
    sites = hrc.open_list(c["L"], lo, hi, words)
    x0 = np.tile(c["wt"], (n, 1))
    for b in range(n):                                        # 4 or more open residues at allowed letters, kept only if free
        for _ in range(200):
            x = c["wt"].copy()
            for l in rng.choice(sites, size=rng.integers(4, len(sites) + 1), replace=False):
                x[l] = rng.choice(np.flatnonzero((int(words[l]) >> np.arange(20)) & 1))
            if motifs.is_free(x[None], pt, c["wt"])[0]:
                x0[b] = x
                break
    assert ((x0 != c["wt"][None]).sum(1) >= 2).all() and motifs.is_free(x0, pt, c["wt"]).all()
    ch, peeks, st_f, _ = _observed_run(toy, lambda ch: ch.set_recombination(every, D), T=T, n=n, x0=x0, seed=seed, patterns=pats, nmut=nmut)
    st = ch.recombination_state()
    ch.close()
    assert st["events"] == T // every
    seen4 = 0
    for s in range(st["events"]):
        it = (s + 1) * every - 1
        X = peeks[it + 1]["idx"]                              # after the event: a rejected pair still holds its parents
        ev = hrc.event(X, c["wt"], sites, s, it, D, seed)
        pa = st["partner"][s]
        assert np.array_equal(pa, ev["partner"]) and np.array_equal(st["lo"][s], ev["lo"]) and np.array_equal(st["hi"][s], ev["hi"])
        a, b = np.minimum(np.arange(n), pa), np.maximum(np.arange(n), pa)
        d = ((st["child_energy"][s][a] - st["pre_energy"][s][a]) + (st["child_energy"][s][b] - st["pre_energy"][s][b])).astype(np.float32)
        assert np.array_equal(st["log_ratio"][s], d)
        plain, margin = hrc.outcomes(st["log_ratio"][s], ev["u"], st["child_dist"][s], pa, st["child_energy"][s], nmut)
        rejected = st["outcome"][s] != 1
        assert np.array_equal(st["child_dist"][s][rejected], ev["child_dist"][rejected])
        free_child = motifs.is_free(ev["children"], pt, c["wt"])
        want, _ = hrc.outcomes(st["log_ratio"][s], ev["u"], st["child_dist"][s], pa, st["child_energy"][s], nmut, pair_free=free_child & free_child[pa])
        sure = rejected & ((margin > 1e-5) | (want >= 2))
        assert np.array_equal(st["outcome"][s][sure], want[sure]), s
        taken = ~rejected
        assert (plain[taken & (margin > 1e-5)] == 1).all()
        seen4 += int((st["outcome"][s] == 4).sum())
    assert seen4 > 0 and (st["outcome"] == 1).any()


# ------------------------------------------------------------------------------------------------ 7. allow_native
def test_allow_native(toy):
    from ppde_amd._hip import PpdeHipError
    c, lib, m, _ = toy
    pt = motifs.parse("F{S}")
    native = np.flatnonzero(motifs.matches(c["wt"][None], pt)[0, 0])
    assert native.tolist() == [13]                            # the wild type matches at one position
    n, T, lo, hi = 64, 40, c["i0"], c["i0"] + c["Lp"] - 1
    ch = _chains(m, c, n, T, 2, 0, 1, lib, pt, True, lo=lo, hi=hi, use_graph=False)
    assert ch.forbidden["note"] is None
    seen_other = False
    for t in range(T):
        ch.run(1)
        idx = ch.peek()["idx"]
        hit = motifs.matches(idx, pt)[:, 0]
        assert not hit[:, np.arange(c["L"]) != 13].any(), t   # the same pattern elsewhere is never accepted
        seen_other |= bool((hit[:, 13] & (idx[:, 14] != c["wt"][14])).any())
    st = ch.forbidden_state()
    assert st["allow_native"] and st["vetoes"].sum() > 0 and not (int(st["active"][13]) & 1) and (int(st["active"][12]) & 1)
    assert seen_other or (idx != c["wt"][None]).any()         # the run proceeds; the native site may hold other matching letters
    ch.close()
    ch = _chains(m, c, n, T, 2, 0, 1, lib, pt, False, lo=lo, hi=hi, init=False)
    assert "pattern 0 at position 13" in ch.forbidden["note"]
    with pytest.raises(PpdeHipError, match=r"\[-1\].*chain 0 is not free: forbidden pattern 0 matches at position 13"):
        ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    x0 = np.tile(c["wt"], (n, 1))
    x0[:, 13] = next(k for k in range(20) if (int(lib[13]) >> k) & 1 and k != int(c["wt"][13]))
    assert motifs.is_free(x0, pt, c["wt"], False).all()
    ch.init(torch.as_tensor(x0).cuda())                       # the run is legal from other free states
    ch.run(T)
    assert motifs.is_free(ch.peek()["idx"], pt, c["wt"], False).all()
    ch.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_object_unchanged(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, m, _ = toy
    n, T, lo, hi, L = 16, 20, c["i0"], c["i0"] + c["Lp"] - 1, c["L"]
    good = motifs.parse(hm.REPLAY_PATTERNS)
    twin = _chains(m, c, n, T, 2, 3, 1, lib, good, lo=lo, hi=hi)
    twin.run(T)
    want = (twin.collect(), twin.forbidden_state()["vetoes"])
    twin.close()

    def P(elements, lengths):
        return motifs.Patterns(np.asarray(elements, dtype=np.uint32), lengths)

    row = lambda *w: list(w) + [0] * (8 - len(w))
    refusals = [
        (P(np.zeros((0, 8)), []), "n_patterns must be in 1..32"),
        (P(np.ones((33, 8)), [1] * 33), "n_patterns must be in 1..32"),
        (P([row(1)], [0]), "pattern 0: length must be in 1..8"),
        (P([row(1), [1] * 8], [1, 9]), "pattern 1: length must be in 1..8"),
        (P([row(1, 0)], [2]), "pattern 0, element 1: empty letter set"),
        (P([row(1, 1 << 20)], [2]), "pattern 0, element 1: a bit >= 20"),
        (P([row((1 << 20) - 1)], [1]), "no active"),
    ]
    ch = _chains(m, c, n, T, 2, 3, 1, lib, good, lo=lo, hi=hi, init=False)
    for pt, msg in refusals:
        with pytest.raises(PpdeHipError, match=r"\[-1\].*" + msg):
            ch.set_forbidden(pt)
    ch.set_forbidden(P([row(1, 1 << 20), row(3)], [1, 1]))    # a word behind the length is ignored; replaces ...
    ch.set_forbidden(P([[1] * 8] * 32, [8] * 32))             # ... the edges M = 32 and length 8 are legal ...
    ch.set_forbidden(None)                                    # ... clears ...
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no patterns were set"):
        ch.forbidden_state()
    ch.set_forbidden(good)                                    # ... and sets again
    with pytest.raises(PpdeHipError, match=r"\[-1\].*pattern constraint is set and needs reversible mode"):
        ch.set_reversible(False)
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_forbidden(good)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_forbidden(None)
    ch.run(T)
    _same(want[0], ch.collect(), RESULT_KEYS, "after the refusals")
    assert np.array_equal(want[1], ch.forbidden_state()["vetoes"])
    ch.close()
    # reversible mode off; a pattern longer than the sequence; a start that is not free
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=99)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*needs reversible mode"):
        ch.set_forbidden(good)
    ch.close()
    short = dict(hr.cap_case())
    ms = hl.hip_model_of(short)
    ch = _chains(ms, short, 4, 4, 2, 0, 1, short["allowed"], None, init=False)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*pattern 0: length 8 exceeds the sequence length 7"):
        ch.set_forbidden("K(8)")
    ch.set_forbidden("K(7)")
    ch.close()
    ms.close()
    x0 = np.tile(c["wt"], (n, 1))
    x0[5, 20:23] = [ALPHABET.index("G"), ALPHABET.index("A"), ALPHABET.index("F")]          # a frozen stretch outside the window
    bad_m, bad_p = (int(v[5]) for v in motifs.find(x0, good, c["wt"]))
    assert bad_m >= 0 and bad_p >= 20
    ch = _chains(m, c, n, T, 2, 3, 1, lib, good, lo=lo, hi=hi, init=False)
    with pytest.raises(PpdeHipError, match=rf"\[-1\].*chain 5 is not free: forbidden pattern {bad_m} matches at position {bad_p}"):
        ch.init(torch.as_tensor(x0).cuda())
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())                               # the refused init left nothing behind
    ch.run(T)
    _same(want[0], ch.collect(), RESULT_KEYS, "after the refused init")
    ch.close()


# ------------------------------------------------------------------------------------------------ 9. PPDE_PAS and the driver
def test_ppde_pas_and_the_driver_end_to_end():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd import synthetic
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    forbid = "deamidation, " + hm.REPLAY_PATTERNS               # a preset in front of the replay cases' patterns
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True, ppde_forbid=forbid)
        en = ProteinProductOfExperts(args)
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        np.random.seed(5)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sampler = PPDE_PAS(args)
            best_x, best_e, best_f, e_hist, f_hist, rtraj = sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10)
        L = len(seq)
        pt = motifs.parse(forbid)
        assert pt.text[0] == "N[GS]" and len(pt) == 4
        np.random.seed(5)
        ch = Chains(en.model, n, T, pas, nmut, False, 0, L - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_library(dl.fold_range(dl.full_library(L), i0, i0 + Lp - 1))
        ch.set_reversible(True)
        ch.set_forbidden(pt)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res, st = ch.collect(), ch.forbidden_state()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"])
        fb = sampler.forbidden
        assert np.array_equal(fb["vetoes"], st["vetoes"]) and fb["text"] == pt.text and fb["allow_native"] and st["vetoes"].sum() > 0
        assert np.array_equal(fb["active"], motifs.active_words(pt, L, en.model.wt_idx, True))
        assert motifs.is_free(res["best_idx"], pt, en.model.wt_idx).all()
        s = motifs.summarise(st["vetoes"], T, pt.text)
        assert fb["summary"]["share"] == s["share"] and "   " + motifs.log_line(s) in buf.getvalue()
        assert "   # forbidden patterns: vetoed 0." in buf.getvalue() and "(N[GS]: 0." in buf.getvalue()
        # the argument checks of PPDE_PAS, before any device work
        for a_, msg in (({"ppde_reversible": False}, "needs ppde_reversible"), ({"ppde_forbid": "NB"}, "column 1"),
                        ({"ppde_forbid": ["NG"] * 33}, "at most 32"), ({"ppde_forbid": None, "ppde_forbid_strict": True}, "needs ppde_forbid")):
            with pytest.raises(ValueError, match=msg):
                PPDE_PAS(argparse.Namespace(**{**vars(args), **a_}))
        native = ALPHABET[int(en.model.wt_idx[0])] + ALPHABET[int(en.model.wt_idx[1])]
        strict = PPDE_PAS(argparse.Namespace(**{**vars(args), "ppde_forbid": native, "ppde_forbid_strict": True}))
        strict._wt_idx = en.model.wt_idx
        with pytest.raises(ValueError, match=r"chain 0 is not free: forbidden pattern 0 \(" + native + r"\) matches at position 0"):
            strict._plan(x0, T, i0, i0 + Lp - 1)
        # the driver with the same flags, the patterns split between the flag and a file
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_motifs", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        res_dir = os.path.join(root, "results")
        more = os.path.join(root, "more_patterns.txt")
        with open(more, "w") as f:
            f.write("# the replay cases' patterns\n" + "\n".join(t.strip() for t in hm.REPLAY_PATTERNS.split(",")) + "\n")
        a = drv.build_parser().parse_args([
            "--protein_weights", root, "--protein", "TOY24", "--results_path", res_dir, "--hub_dir", res_dir, "--device", "cuda:0",
            "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--n_chains", str(n), "--n_iters", str(T), "--seed", "3",
            "--log_every", "10", "--energy_lamda", "5", "--nmut_threshold", str(nmut), "--ppde_rng", "philox", "--ppde_seed", str(seed),
            "--ppde_reversible", "--ppde_forbid", "deamidation", "--ppde_forbid_file", more, "--run_signature", "motifs"])
        a.ppde_reuse_grad = True
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            out = drv.main(a)
        have = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
        assert {"motif_vetoes.npy", "motif_patterns.txt"} <= have
        v = np.load(os.path.join(out, "motif_vetoes.npy"))
        assert v.shape == (n, 4) and v.dtype == np.int64 and np.array_equal(v, st["vetoes"])     # the same seed: the same run
        assert open(os.path.join(out, "motif_patterns.txt")).read().split() == pt.text
        assert "   " + motifs.log_line(s) in log.getvalue()

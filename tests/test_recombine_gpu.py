"""Recombination on the GPU (ppde_chains_set_recombination; k_cross_propose, k_cross_accept): up to the first event the run is the
reversible run, event 0 is the rule of tests/helpers_recombine.py on the plain run's population, later events are consistent with
their own records, graph replay (aligned and misaligned) equals the stepped twin, both gradient policies give the same bits, the
joint law of a deme follows the enumerated kernels and the exact pair matrix, the observers keep their rules, sharding changes
nothing, the refusals, PPDE_PAS and the driver end to end, a transformer geometry, and a replay of the CPU reference run.

Discrete results are compared exactly; everything the device derives from its OWN numbers (pre_energy against the history,
log_ratio against the recorded energies, a taken child against child_energy, graph against stepped, the two gradient policies) bit
for bit; child_energy against the stateless evaluation of the children within 5e-6 max(1, |e|) + 5e-6 lamda."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_anneal as ha
import helpers_library as hl
import helpers_recombine as hrc
import helpers_reversible as hr
import helpers_tempering as ht
from ppde_amd import library as dl
from ppde_amd import recombine as rcb

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
PEEK_KEYS = ("idx", "energy", "fitness", "accepted", "dist")
EVENT_KEYS = ("partner", "lo", "hi", "differ", "child_dist", "outcome", "log_ratio", "pre_energy", "child_energy")


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, every=0, deme=0, x0=None, lo=None, hi=None, which=None, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", 99)
    lo = 0 if lo is None else lo
    hi = case["L"] - 1 if hi is None else hi
    which = (3 if case.get("cnn") is not None else 1) if which is None else which
    ch = Chains(m, n, T, pas, nmut, False, lo, hi, which, rng_mode, **kw)
    if lib is not None:
        ch.set_library(lib)
    ch.set_reversible(True)
    if every:
        ch.set_recombination(every, deme)
    x0 = np.tile(case["wt"], (n, 1)) if x0 is None else x0
    ch.init(torch.as_tensor(x0).cuda())
    return ch


def _stepped(ch, T):
    peeks = [ch.peek()]
    for _ in range(T):
        ch.run(1)
        peeks.append(ch.peek())
    return peeks


def _same(a, b, keys, label):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def _noise(rng_mode, n, c, T, seed=77):
    import ppde_oracle as orc
    if rng_mode != 0:
        return None
    gen = torch.Generator().manual_seed(seed)
    return [orc.draw_noise_torch(n, c["L"] * 20, 2, generator=gen) for _ in range(T)]


def _run(ch, T, noise, first=0):
    if noise is None:
        ch.run(T)
        return
    for U, q, u in noise[first:first + T]:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _scattered(c, lib, n, lo, hi, seed, most=3):
    """Start states that differ between the chains: up to `most` open residues of each chain at another allowed letter."""
    rng = np.random.default_rng(seed)
    words = dl.as_words(lib, c["L"])
    sites = hrc.open_list(c["L"], lo, hi, words)
    x0 = np.tile(c["wt"], (n, 1))
    for b in range(n):
        for l in rng.choice(sites, size=rng.integers(0, most + 1), replace=False):
            x0[b, l] = rng.choice(np.flatnonzero((int(words[l]) >> np.arange(20)) & 1))
    return x0


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, m
    m.close()


# ------------------------------------------------------------------------------------------------ 1. before the first event
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_up_to_the_first_event_nothing_changes(toy, rng_mode):
    """12 chains, D = 4, every = 7, T = 20: history rows 0..6 and the traces of iterations 0..5 equal the plain reversible run's
    bit for bit (whose reuse run on the device RNG goes through the fused kernel)."""
    c, lib, m = toy
    n, T, every, lo, hi = 12, 20, 7, c["i0"], c["i0"] + c["Lp"] - 1
    noise = _noise(rng_mode, n, c, T)
    out = []
    for ev in (0, every):
        ch = _chains(m, c, n, T, 2, 3, rng_mode, lib, ev, 4, lo=lo, hi=hi, trace=True)
        _run(ch, T, noise)
        out.append((ch.collect(), ch.trace()))
        if ev:
            st = ch.recombination_state()
            assert st["events"] == 2 and ch.recombination_shape()[0] == 4 and ch.recombination_shape()[2] == 2
        ch.close()
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(out[0][0][k][:every], out[1][0][k][:every]), k
    assert np.array_equal(out[0][0]["random_traj"][:every], out[1][0]["random_traj"][:every])
    for k in ("flat", "accepted", "log_acc", "U"):
        assert np.array_equal(out[0][1][k][:every - 1], out[1][1][k][:every - 1]), k
    assert out[0][1]["accepted"][:every - 1].any()


# ------------------------------------------------------------------------------------------------ 2. event 0 is the rule
def _check_event0(m, c, lib, which, nmut, n, D, every, seed, x0, lo, hi, lamda, off=0):
    T = every
    plain = _chains(m, c, n, T, 2, nmut, 1, lib, 0, 0, x0=x0, lo=lo, hi=hi, which=which, seed=seed, chain_offset=off)
    plain.run(T)
    P, R = plain.peek(), plain.collect()
    plain.close()
    ch = _chains(m, c, n, T, 2, nmut, 1, lib, every, D, x0=x0, lo=lo, hi=hi, which=which, seed=seed, chain_offset=off)
    ch.run(T)
    Q, S_, st = ch.peek(), ch.collect(), ch.recombination_state()
    ch.close()
    sites = hrc.open_list(c["L"], lo, hi, None if lib is None else dl.as_words(lib, c["L"]))
    assert np.array_equal(st["open_sites"], sites) and st["events"] == 1 and st["deme"] == D
    ev = hrc.event(P["idx"], c["wt"], sites, 0, every - 1, D, seed, off)
    for k in ("partner", "lo", "hi", "differ", "child_dist"):
        assert np.array_equal(st[k][0], ev[k]), k
    assert np.array_equal(st["pre_energy"][0], R["energy_history"][every])
    pa = ev["partner"]
    ce, pe = st["child_energy"][0], st["pre_energy"][0]
    a = np.minimum(np.arange(n), pa)
    b = np.maximum(np.arange(n), pa)
    d32 = (ce[a] - pe[a]) + (ce[b] - pe[b])
    assert d32.dtype == np.float32 and np.array_equal(st["log_ratio"][0], d32)
    e_ref, f_ref, _ = m.energy_grad(torch.as_tensor(ev["children"].astype(np.uint8)), which, want_grad=False)
    e_ref, f_ref = e_ref.cpu().numpy(), f_ref.cpu().numpy()
    tol = 5e-6 * np.maximum(1.0, np.abs(e_ref)) + 5e-6 * lamda
    print(f"recombination event 0: child energy worst {np.abs(ce - e_ref).max():.3g} (tolerance from {tol.min():.3g})")
    assert (np.abs(ce - e_ref) <= tol).all()
    want, margin = hrc.outcomes(st["log_ratio"][0], ev["u"], ev["child_dist"], pa, ce, nmut)
    close = margin <= 2.0 ** -22
    assert close.sum() <= 2, "at most one decision (both slots of one pair) may sit on the rounding of expf"
    assert np.array_equal(st["outcome"][0][~close], want[~close])
    acc = st["outcome"][0] == 1
    assert np.array_equal(Q["idx"], np.where(acc[:, None], ev["children"], P["idx"]))
    assert np.array_equal(Q["energy"], np.where(acc, ce, pe)) and np.array_equal(S_["energy_history"][every], Q["energy"])
    assert np.array_equal(Q["dist"], np.where(acc, ev["child_dist"], P["dist"]))
    assert np.array_equal(Q["accepted"], P["accepted"])                       # the slot's own Metropolis result
    assert np.array_equal(S_["energy_history"][:every], R["energy_history"][:every])
    better = acc & (ce > R["best_energy"])
    assert np.array_equal(S_["best_idx"], np.where(better[:, None], ev["children"], R["best_idx"]))
    assert np.array_equal(S_["best_step"], np.where(better, every, R["best_step"]))
    assert np.array_equal(S_["best_energy"], np.where(better, ce, R["best_energy"]))
    assert np.array_equal(S_["random_traj"][every], Q["idx"][0]) and np.array_equal(S_["random_traj"][:every], R["random_traj"][:every])
    return st, ev


@pytest.mark.parametrize("which", [1, 3])
def test_event_0_is_the_rule(toy, which):
    """12 chains in demes of 4 from scattered start states, every = 3, a shard that starts at chain 8: Potts only, and Potts + CNN."""
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, 12, lo, hi, seed=3)
    st, ev = _check_event0(m, c, lib, which, 0, 12, 4, 3, 1234, x0, lo, hi, float(c["lamda"]) if which == 3 else 0.0, off=8)
    assert (st["outcome"][0] == 1).any() and (ev["differ"] > 0).any()
    assert (st["outcome"][0][ev["differ"] == 0] == 1).all()


def test_event_0_with_a_cap_rejects_the_capped_children(toy):
    """The same with nmut = 3 and start states at up to two mutations: some child reaches the cap, outcome 2 for both slots."""
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, 24, lo, hi, seed=11, most=2)
    st, ev = _check_event0(m, c, lib, 3, 3, 24, 6, 2, 4321, x0, lo, hi, float(c["lamda"]))
    assert (st["outcome"][0] == 2).any(), "pick start states from which some child reaches the cap"
    assert (st["outcome"][0] == 1).any()


# ------------------------------------------------------------------------------------------------ 3. later events
def test_later_events_are_self_consistent(toy):
    c, lib, m = toy
    n, T, every, D, lo, hi = 12, 24, 4, 6, c["i0"], c["i0"] + c["Lp"] - 1
    ch = _chains(m, c, n, T, 2, 0, 1, lib, every, D, x0=_scattered(c, lib, n, lo, hi, seed=5), lo=lo, hi=hi, use_graph=False)
    peeks = _stepped(ch, T)
    res, st = ch.collect(), ch.recombination_state()
    ch.close()
    assert st["events"] == T // every and (st["outcome"] == 1).any() and (st["outcome"] == 0).any()
    sites, lam = st["open_sites"], float(c["lamda"])
    for e in range(st["events"]):
        t = (e + 1) * every
        assert np.array_equal(st["partner"][e], (np.arange(n) // D) * D + np.tile(hrc.partners(e, D), n // D))
        acc = st["outcome"][e] == 1
        post = peeks[t]["idx"]
        parents = post.copy()
        for i in np.flatnonzero(acc):
            seg = sites[st["lo"][e, i]:st["hi"][e, i] + 1]
            parents[i, seg] = post[st["partner"][e, i], seg]
        e_ref = m.energy_grad(torch.as_tensor(parents), 3, want_grad=False)[0].cpu().numpy()
        assert (np.abs(e_ref - st["pre_energy"][e]) <= 5e-6 * np.maximum(1.0, np.abs(e_ref)) + 5e-6 * lam).all()
        assert np.array_equal(res["energy_history"][t], np.where(acc, st["child_energy"][e], st["pre_energy"][e]))
        assert np.array_equal(peeks[t]["energy"], res["energy_history"][t])
        assert np.array_equal((parents != c["wt"][None]).sum(1)[~acc], peeks[t]["dist"][~acc])
        assert np.array_equal((post != c["wt"][None]).sum(1), peeks[t]["dist"])


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("every,runs,replayed", [(10, (120, 20, 7), 140), (7, (3, 100, 44), 91 + 42)])
def test_graph_replay_equals_the_stepped_twin(toy, every, runs, replayed):
    """12 chains, D = 6, T = 147. every = 10 (segments of 100 and 10): 120 + 20 + 7 replays 100 + 2 x 10, 2 x 10, nothing.
    every = 7 (segments of 98 and 7): 3 eager; 4 eager to position 7, 13 x 7 replayed, 5 eager; 2 eager to 105, 6 x 7 replayed."""
    c, lib, m = toy
    n, T, D, lo, hi = 12, 147, 6, c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, n, lo, hi, seed=9)
    twin = _chains(m, c, n, T, 2, 3, 1, lib, every, D, x0=x0, lo=lo, hi=hi, use_graph=False)
    peeks = _stepped(twin, T)
    res, st = twin.collect(), twin.recombination_state()
    twin.close()
    ch = _chains(m, c, n, T, 2, 3, 1, lib, every, D, x0=x0, lo=lo, hi=hi)
    done = 0
    for k in runs:
        ch.run(k)
        done += k
        _same(ch.peek(), peeks[done], PEEK_KEYS, f"after {done}")
    gs = ch.graph_stats()
    assert gs["replayed_steps"] == replayed and gs["eager_steps"] == T - replayed and gs["captures_in_run"] == 0
    _same(ch.collect(), res, RESULT_KEYS, "graph against stepped")
    _same(ch.recombination_state(), st, EVENT_KEYS, "graph against stepped")
    ch.close()
    assert st["events"] == T // every and ((st["outcome"] == 1) & (st["differ"] > 0)).any()


# ------------------------------------------------------------------------------------------------ 5. the gradient policies
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_both_gradient_policies_give_the_same_bits(toy, rng_mode):
    """Re-evaluating against reuse (whose next proposal reads grad_cur: the child's combined row), and reuse with and without graphs."""
    c, lib, m = toy
    n, T, every, D, lo, hi = 12, 30, 3, 4, c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, n, lo, hi, seed=21)
    noise = _noise(rng_mode, n, c, T)
    out = []
    for reuse, graph in ((False, False), (True, False), (True, True)):
        ch = _chains(m, c, n, T, 2, 3, rng_mode, lib, every, D, x0=x0, lo=lo, hi=hi, reuse_grad=reuse, use_graph=graph, trace=True)
        _run(ch, T, noise)
        out.append((ch.collect(), ch.peek(), ch.recombination_state(), ch.trace()))
        ch.close()
    for o in out[1:]:
        _same(out[0][0], o[0], RESULT_KEYS, "policies")
        _same(out[0][1], o[1], PEEK_KEYS, "policies")
        _same(out[0][2], o[2], EVENT_KEYS, "policies")
        _same(out[0][3], o[3], ("flat", "accepted", "log_acc", "U"), "policies")
    assert ((out[0][2]["outcome"] == 1) & (out[0][2]["differ"] > 0)).sum() >= 3


# ------------------------------------------------------------------------------------------------ 6. the law
_LAW = {}


def _law_case(name, case):
    if name not in _LAW:
        en = hl.oracle_energy_of(case)
        K, states, index, _, inside = hr.exact_reversible_kernel(en, case["wt"], case["allowed"], 2, 0, case["L"] - 1, case.get("nmut", 0))
        e32, _ = en.energy(states)
        positions = np.flatnonzero(case["allowed"])
        _LAW[name] = (K, states, index, inside, hrc.pair_matrix(states.numpy(), positions, e32.numpy(), inside))
    return _LAW[name]


def _demes_against(label, m, c, every, D, n_demes, T, start_rows, expected, states, index, seed):
    S = states.shape[0]
    x0 = np.tile(np.stack([states[s].numpy().astype(np.uint8) for s in start_rows]), (n_demes, 1))
    ch = _chains(m, c, n_demes * D, max(T, every), 2, c["nmut"], 1, c["allowed"], every, D, x0=x0, random_chain=-1, seed=seed)
    ch.run(T)
    idx = ch.peek()["idx"]
    ch.close()
    cells, forbidden = ha.deme_cells(idx, D, c["allowed"], index, states[start_rows[0]].numpy(), S)
    assert forbidden == 0
    chi2, df = hl.chi_square(np.bincount(cells, minlength=S ** D).astype(np.float64), n_demes * expected)
    print(f"recombination law, {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)


def _wt_row(c, index):
    return index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]


@pytest.mark.parametrize("nmut", [0, 2])
@pytest.mark.parametrize("every", hrc.LAW_EVERY)
def test_law_of_pairs(every, nmut):
    """Case A (35 states, two open residues), 2^16 pairs, T in 1, 2, 3, 8 from the wild type and from the power start, against
    helpers_recombine.joint_law_recombined; and the same with nmut = 2 (11 states under the cap)."""
    c = dict(ht.case_a(), nmut=nmut)
    K, states, index, inside, X = _law_case(("A", nmut), c)
    m = hl.hip_model_of(c)
    S, w = states.shape[0], _wt_row(c, index)
    for T in hrc.LAW_T:
        for start in ((w, w), POWER_START_A[nmut]):
            expected = hrc.joint_law_recombined(T, K, X, every, 2, start[0] * S + start[1])
            _demes_against(f"case A nmut={nmut}: T={T} every={every} start={start}", m, c, every, 2, 1 << 16, T, start, expected,
                           states, index, seed=7977 + 13 * T + every + start[0])
    m.close()


@pytest.mark.parametrize("every", hrc.LAW_EVERY)
def test_law_of_demes_of_four(every):
    """Case C (8 states, three open residues), 2^15 demes of 4."""
    c = hrc.case_c()
    K, states, index, inside, X = _law_case("C", c)
    m = hl.hip_model_of(c)
    S, w = states.shape[0], _wt_row(c, index)
    for T in hrc.LAW_T:
        for start in ((w,) * 4, POWER_START_C):
            j0 = int(np.ravel_multi_index(start, (S,) * 4))
            expected = hrc.joint_law_recombined(T, K, X, every, 4, j0)
            _demes_against(f"case C: T={T} every={every} start={start}", m, c, every, 4, 1 << 15, T, start, expected, states, index,
                           seed=8977 + 13 * T + every)
    m.close()


POWER_START_A, POWER_START_C = hrc.POWER_START_A, hrc.POWER_START_C


# ------------------------------------------------------------------------------------------------ 8. sharding
def test_sharding_does_not_change_a_recombination_run(toy):
    """16 chains as 4 + 12 with D = 4 against one object; partners compared as global indices."""
    c, lib, m = toy
    T, lo, hi = 12, c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, 16, lo, hi, seed=31)

    def run(n_, off):
        ch = _chains(m, c, n_, T, 2, 3, 1, lib, 3, 4, x0=x0[off:off + n_], lo=lo, hi=hi, chain_offset=off, random_chain=0 if off == 0 else -1)
        ch.run(T)
        r, st, p = ch.collect(), ch.recombination_state(), ch.peek()
        ch.close()
        return r, st, p

    (one, st1, p1), (a, sta, pa), (b, stb, pb) = run(16, 0), run(4, 0), run(12, 4)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    for k in PEEK_KEYS:
        assert np.array_equal(np.concatenate([pa[k], pb[k]], 0), p1[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    assert np.array_equal(np.concatenate([sta["partner"], stb["partner"] + 4], 1), st1["partner"])
    for k in EVENT_KEYS[1:]:
        assert np.array_equal(np.concatenate([sta[k], stb[k]], 1), st1[k]), k
    assert ((st1["outcome"] == 1) & (st1["differ"] > 0)).any()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_set_recombination_refusals_at_their_edges(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    T = 20
    wt8 = torch.as_tensor(np.tile(c["wt"], (8, 1))).cuda()

    def fresh(n=8, **kw):
        return Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7, **kw)

    ch = fresh()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*needs reversible mode"):                 # reversible mode is not on
        ch.set_recombination(1, 4)
    ch.set_reversible(True)
    for every, deme, what in ((1, 3, "even and >= 2"), (1, 1, "even and >= 2"), (1, -2, "even and >= 2"),      # D odd, D < 2
                              (1, 6, "n_chains must be a multiple"), (-1, 4, "every must be >= 1"), (T + 1, 4, "no event would fit")):
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
            ch.set_recombination(every, deme)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no recombination was set"):
        ch.recombination_shape()
    ch.set_tempering((1.0, 0.5), 1)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*tempering is set"):
        ch.set_recombination(1, 4)
    ch.set_tempering(None)
    ch.set_annealing((0.5, 1.0), 1, 4)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set"):
        ch.set_recombination(1, 4)
    ch.set_annealing(None)
    ch.set_recombination(T, 2)                                                # the accepted edges: D = 2, one event at the very end
    ch.set_recombination(1, 8)                                                # replaced
    for call, what in ((lambda: ch.set_library(lib), "recombination is set"), (lambda: ch.set_library(None), "recombination is set"),
                       (lambda: ch.set_tempering((1.0, 0.5), 1), "recombination is set"),
                       (lambda: ch.set_annealing((0.5, 1.0), 1, 4), "recombination is set"),
                       (lambda: ch.set_reversible(False), "recombination is set and needs reversible mode")):
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
            call()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*not initialised"):
        ch.recombination_shape()
    ch.set_recombination(None)                                                # cleared: everything is allowed again
    ch.set_library(lib)
    ch.set_reversible(False)
    ch.init(wt8)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_recombination(1, 4)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no recombination was set"):
        ch.recombination_state()
    ch.close()
    for off, what in ((6, "chain_offset must be a multiple"), (0, None)):
        ch = fresh(8, chain_offset=off)
        ch.set_library(lib)
        ch.set_reversible(True)
        if what:
            with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
                ch.set_recombination(1, 4)
        else:
            ch.set_recombination(2, 4)
            ch.init(wt8)
            ch.run(3)
            with pytest.raises(PpdeHipError, match=r"\[-1\].*events beyond"):
                ch.recombination_state(0, 2)
            st = ch.recombination_state()
            assert st["events"] == 1 and ch.recombination_shape()[2:] == (T // 2, 1)
            assert np.array_equal(st["open_sites"], hrc.open_list(c["L"], lo, hi, dl.as_words(lib, c["L"])))
        ch.close()
    ch = fresh(n_streams=2)
    ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_recombination(1, 4)
    ch.close()


# ------------------------------------------------------------------------------------------------ lineage on a real run
def test_lineage_of_a_run_agrees_with_exchanging_founder_labels_by_hand(toy):
    """8 chains in demes of 4, an event behind every one of 6 iterations: ppde_amd.recombine.lineage on the device's records equals
    founder labels exchanged pair by pair over the recorded accepted segments."""
    c, lib, m = toy
    n, T, lo, hi = 8, 6, c["i0"], c["i0"] + c["Lp"] - 1
    x0 = _scattered(c, lib, n, lo, hi, seed=41)
    ch = _chains(m, c, n, T, 2, 0, 1, lib, 1, 4, x0=x0, lo=lo, hi=hi, use_graph=False)
    peeks = _stepped(ch, T)
    st = ch.recombination_state()
    ch.close()
    who = rcb.lineage(st, st["open_sites"], n, c["L"])
    lab = np.tile(np.arange(n)[:, None], (1, c["L"]))
    for e in range(st["events"]):
        for a_ in range(n):
            b_ = st["partner"][e, a_]
            if a_ < b_ and st["outcome"][e, a_] == 1:
                seg = st["open_sites"][st["lo"][e, a_]:st["hi"][e, a_] + 1]
                lab[a_, seg], lab[b_, seg] = lab[b_, seg].copy(), lab[a_, seg].copy()
    assert np.array_equal(who, lab) and (who != np.arange(n)[:, None]).any()
    assert rcb.summarise(st)["pairs"] == T * n // 2


# ------------------------------------------------------------------------------------------------ 7. the observers
def test_observers_keep_their_rules_on_the_recombined_population(toy):
    """Recorder rows, site and pair counts, archive and move statistics of a recombination run (graph replay) equal their own rules
    applied to the peeks of the stepped twin without them."""
    import helpers_archive as har
    import helpers_pairs as hp
    import helpers_stats as hs
    c, lib, m = toy
    n, T, lo, hi, D, every = 12, 20, c["i0"], c["i0"] + c["Lp"] - 1, 6, 4
    x0 = _scattered(c, lib, n, lo, hi, seed=51)
    twin = _chains(m, c, n, T, 2, 3, 1, lib, every, D, x0=x0, lo=lo, hi=hi, seed=77, trace=True, use_graph=False)
    peeks = _stepped(twin, T)
    tr, res, st = twin.trace(), twin.collect(), twin.recombination_state()
    twin.close()
    sites = np.arange(lo, hi + 1, dtype=np.int32)
    from ppde_amd.sampler import Chains
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, random_chain=0, seed=77)
    ch.set_library(lib)
    ch.set_reversible(True)
    ch.set_recombination(every, D)
    ch.set_recorder(1, 0, None, True)
    ch.set_pair_counts(sites)
    ch.set_archive(3)
    ch.set_stats(True)
    ch.init(torch.as_tensor(x0).cuda())
    ch.run(T)
    assert ch.graph_stats()["replayed_steps"] == T
    _same(ch.collect(), res, RESULT_KEYS, "observers change nothing")
    _same(ch.recombination_state(), st, EVENT_KEYS, "observers change nothing")
    rec, (pc, ps), arc, stats = ch.recorded(), ch.pair_counts(), ch.archive(), ch.stats()
    ch.close()
    assert ((st["outcome"] == 1) & (st["differ"] > 0)).any()
    assert rec["rows"] == T
    for t in range(1, T + 1):
        assert np.array_equal(rec["idx"][t - 1], peeks[t]["idx"]) and np.array_equal(rec["energy"][t - 1], peeks[t]["energy"])
        assert np.array_equal(rec["fitness"][t - 1], peeks[t]["fitness"])
    allidx = np.stack([p["idx"] for p in peeks[1:]])
    counts = np.zeros((c["L"], 20), np.uint64)
    for l in range(c["L"]):
        counts[l] = np.bincount(allidx[:, :, l].reshape(-1), minlength=20)
    assert np.array_equal(rec["site_counts"], counts)
    assert np.array_equal(ps, sites) and np.array_equal(pc, hp.pair_counts_of(allidx, sites))
    want = har.archive_of(peeks, 3)
    for k in ("idx", "energy", "fitness", "step", "count"):
        assert np.array_equal(arc[k], want[k]), k
    ws = hs.stats_of(peeks, tr["accepted"], tr["U"], None, 0, 3)
    for k in hs.KEYS:
        assert np.array_equal(stats[k], ws[k]), k


# ------------------------------------------------------------------------------------------------ 10. PPDE_PAS and the driver
def test_ppde_pas_runs_the_chains_a_caller_would_build_by_hand():
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
    n, T, pas, nmut, seed, every, D = 8, 20, 2, 3, 4242, 5, 4
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True, ppde_recombine_every=every, ppde_recombine_deme=D)
        en = ProteinProductOfExperts(args)
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        np.random.seed(5)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sampler = PPDE_PAS(args)
            best_x, best_e, best_f, e_hist, f_hist, rtraj = sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10)
        L = len(seq)
        np.random.seed(5)
        ch = Chains(en.model, n, T, pas, nmut, False, 0, L - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_library(dl.fold_range(dl.full_library(L), i0, i0 + Lp - 1))
        ch.set_reversible(True)
        ch.set_recombination(every, D)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res, st = ch.collect(), ch.recombination_state()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(f_hist, res["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"]) and np.array_equal(best_e, res["best_energy"])
        rc = sampler.recombination
        assert rc["deme"] == D and rc["every"] == every and rc["events"] == T // every == st["events"]
        assert np.array_equal(rc["open_sites"], np.arange(i0, i0 + Lp))
        for k in EVENT_KEYS:
            assert np.array_equal(rc[k], st[k]), k
        assert np.array_equal(rc["cut"], np.stack([st["lo"], st["hi"]], -1))
        assert rc["summary"] == rcb.summarise(st)
        assert "   # recombination: event 2, accepted " in buf.getvalue() and "   # recombination: event 4, accepted " in buf.getvalue()
        for a_ in ({"ppde_reversible": False}, {"ppde_betas": (1.0, 0.5)}, {"ppde_anneal_betas": (0.5, 1.0)}, {"ppde_recombine_deme": 3},
                   {"ppde_streams": 2}, {"ppde_recombine_every": -1}):
            with pytest.raises(ValueError, match="ppde_recombine"):
                PPDE_PAS(argparse.Namespace(**{**vars(args), **a_}))
        for a_, steps in (({"ppde_recombine_deme": 6}, T), ({}, every - 1)):        # seen with the population, before any device work
            with pytest.raises(ValueError, match="ppde_recombine"):
                PPDE_PAS(argparse.Namespace(**{**vars(args), **a_}))._plan(x0, steps, i0, i0 + Lp - 1)
        # the driver with the same flags: its recombination files, and the lineage read from them
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_recombine", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        res_dir = os.path.join(root, "results")
        a = drv.build_parser().parse_args([
            "--protein_weights", root, "--protein", "TOY24", "--results_path", res_dir, "--hub_dir", res_dir, "--device", "cuda:0",
            "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--n_chains", str(n), "--n_iters", str(T), "--seed", "3",
            "--log_every", "10", "--energy_lamda", "5", "--nmut_threshold", str(nmut), "--ppde_rng", "philox", "--ppde_seed", str(seed),
            "--ppde_reversible", "--ppde_recombine_every", str(every), "--ppde_recombine_deme", str(D), "--run_signature", "recombine"])
        a.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(a)
        E = T // every
        shapes = {"recomb_partner.npy": (E, n), "recomb_cut.npy": (E, n, 2), "recomb_differ.npy": (E, n), "recomb_outcome.npy": (E, n),
                  "recomb_log_ratio.npy": (E, n), "recomb_pre_energy.npy": (E, n), "recomb_child_energy.npy": (E, n),
                  "recomb_open_sites.npy": (Lp,)}
        have = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
        assert set(shapes) <= have, sorted(set(shapes) - have)
        got = {f: np.load(os.path.join(out, f)) for f in shapes}
        for f, shape in shapes.items():
            assert got[f].shape == shape, f
        assert np.array_equal(got["recomb_pre_energy.npy"], st["pre_energy"])     # the same seed: the same run
        recs = dict(partner=got["recomb_partner.npy"], lo=got["recomb_cut.npy"][..., 0], hi=got["recomb_cut.npy"][..., 1],
                    outcome=got["recomb_outcome.npy"])
        who = rcb.lineage(recs, got["recomb_open_sites.npy"], n, L)
        lab = np.tile(np.arange(n)[:, None], (1, L))
        for e in range(E):
            for s_ in range(n):
                p_ = recs["partner"][e, s_]
                if s_ < p_ and recs["outcome"][e, s_] == 1:
                    seg = got["recomb_open_sites.npy"][recs["lo"][e, s_]:recs["hi"][e, s_] + 1]
                    lab[s_, seg], lab[p_, seg] = lab[p_, seg].copy(), lab[s_, seg].copy()
        assert np.array_equal(who, lab)


# ------------------------------------------------------------------------------------------------ 11. the transformer expert
def test_transformer_geometry_gives_equal_bits_under_both_policies():
    """tests/test_modes_gpu.py's toy transformer geometry (Potts + CNN + transformer, which = 7), 8 chains in demes of 4, events
    every 2 of 6 iterations: the re-evaluating and the reuse run agree bit for bit, records included."""
    import helpers_modes as hm
    from ppde_amd.energy import HipModel
    wt, J, h, cnn, tf_state = hm.toy_parts()
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, hm.TOY["win"][0])
    m.set_cnn(cnn)
    m.set_transformer(tf_state, hm.TOY["heads"])
    m.set_lamda(hm.LAMDA)
    c = dict(L=hm.TOY["L"], wt=wt, cnn=cnn)
    lib = hm.window_library(wt, hm.TOY["win"])
    n, T = 8, 6
    x0 = _scattered(c, lib, n, 0, c["L"] - 1, seed=61)
    out = []
    for reuse in (False, True):
        ch = _chains(m, c, n, T, 2, 3, 1, lib, 2, 4, x0=x0, which=7, reuse_grad=reuse)
        ch.run(T)
        out.append((ch.collect(), ch.peek(), ch.recombination_state()))
        ch.close()
    m.close()
    _same(out[0][0], out[1][0], RESULT_KEYS, "transformer")
    _same(out[0][1], out[1][1], PEEK_KEYS, "transformer")
    _same(out[0][2], out[1][2], EVENT_KEYS, "transformer")
    assert out[0][2]["events"] == 3 and (out[0][2]["outcome"] == 1).any()


# ------------------------------------------------------------------------------------------------ replay of the CPU reference
@pytest.mark.parametrize("every,deme", [(1, 2), (3, 4), (2, 12)])
def test_the_device_run_replays_the_cpu_reference(toy, every, deme):
    """TOY24, 12 chains from scattered start states, T = 9: helpers_recombine.recombined_run fed the device's own noise and the
    cuts restated from Philox. States after every iteration, accept bits and the discrete records exact; energies to
    tests/test_tempering_gpu.py's replay tolerances (2e-5 energy, 5e-6 fitness); no decision of the reference near a tie."""
    from helpers import device_noise
    c, lib, m = toy
    en = hl.oracle_energy_of(c)
    n, T, lo, hi, seed = 12, 9, c["i0"], c["i0"] + c["Lp"] - 1, 233
    x0 = _scattered(c, lib, n, lo, hi, seed=71)
    ch = _chains(m, c, n, T, 2, 3, 1, lib, every, deme, x0=x0, lo=lo, hi=hi, seed=seed, trace=True, reuse_grad=False, use_graph=False)
    peeks = _stepped(ch, T)
    tr, res, st = ch.trace(), ch.collect(), ch.recombination_state()
    noise = device_noise(ch, T, 2)
    ch.close()
    ref = hrc.recombined_run(en, x0.astype(np.int64), c["wt"], lambda t: noise[t], T, lo, hi, 2, 3, every, deme, seed, lib)
    u = np.stack([hrc.cut(seed, np.minimum(np.arange(n), ref["partner"][e]), (e + 1) * every - 1, len(st["open_sites"]))[2]
                  for e in range(st["events"])])
    decided = ref["outcome"] < 2
    with np.errstate(over="ignore"):
        margin = np.abs(np.exp(ref["log_ratio"].astype(np.float64)) - u)[decided].min()
    print(f"recombination replay every={every} D={deme}: decision margin {margin:.3g}, accepted "
          f"{int(((st['outcome'] == 1) & (st['differ'] > 0)).sum())} slots in {st['events']} events")
    assert margin > 1e-4, "the reference's own decision sits near a tie: pick another seed"
    assert st["events"] == T // every == ref["partner"].shape[0]
    for t in range(T + 1):
        assert np.array_equal(peeks[t]["idx"], ref["states"][t]), t
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"])
    for k in ("partner", "lo", "hi", "differ", "child_dist", "outcome"):
        assert np.array_equal(st[k], ref[k]), k
    assert ((st["outcome"] == 1) & (st["differ"] > 0)).any(), "a replay in which nothing is ever exchanged shows nothing"
    assert np.abs(res["energy_history"] - ref["energy_history"]).max() <= 2e-5
    assert np.abs(res["fitness_history"] - ref["fitness_history"]).max() <= 5e-6
    for k in ("pre_energy", "child_energy"):
        assert np.abs(st[k] - ref[k]).max() <= 2e-5, k

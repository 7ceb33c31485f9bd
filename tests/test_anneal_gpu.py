"""Population annealing on the GPU (ppde_chains_set_annealing; k_propose_temp, k_accept_temp, k_select_plan, k_select_copy): a
schedule of ones is the reversible run bit for bit, a power-of-two schedule replays the reference of tests/helpers_anneal.py,
the device's plan is the fp64 plan on its own recorded energies, a replaced slot holds its parent's post-accept row, graph replay
equals eager issue, the joint law of a deme follows the enumerated kernels and selection matrices, the observers keep their
rules on the selected population, sharding changes nothing, and the refusals.

Discrete results (states, accept bits, parents, temperatures) are compared exactly. Energies of a device run against the CPU
reference agree to tests/test_tempering_gpu.py's replay tolerances (2e-5 energy, 5e-6 fitness: the device's fp32 sums are not the
oracle's bits); everything the device derives from its OWN energies (pre_energy against the history, a replaced slot against its
parent, the two gradient policies, graph against eager) is compared bit for bit. The law tests use tests/test_sampler_law.py's
statistic and bound; joint cells are (state of slot 0, state of slot 1, ...)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_anneal as ha
import helpers_archive as har
import helpers_library as hl
import helpers_pairs as hp
import helpers_reversible as hr
import helpers_stats as hs
import helpers_tempering as ht
from helpers import device_noise
from ppde_amd import library as dl

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
PEEK_KEYS = ("idx", "energy", "fitness", "accepted", "dist")
EVENT_KEYS = ("parent", "pre_energy", "log_mean_w", "ess", "beta")


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, sched=None, every=1, deme=None, x0=None, lo=None, hi=None, which=None,
            observers=None, **kw):
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
    if sched is not None:
        ch.set_annealing(sched, every, deme)
    if observers:
        ch.set_recorder(1, 0, None, True)
        ch.set_pair_counts(observers["sites"])
        ch.set_archive(observers["K"])
        ch.set_stats(True)
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


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, hl.oracle_energy_of(c), m
    m.close()


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_a_schedule_of_ones_is_the_reversible_run(toy, rng_mode):
    """TOY24, 16 chains in one deme, beta = (1, 1, 1, 1) with a stage behind every fourth iteration, both gradient policies:
    histories, bests, peek and traces equal the reversible run's bit for bit (whose reuse run on the device RNG goes through the
    fused kernel), every parent is its own slot, every ESS is D."""
    import ppde_oracle as orc
    c, lib, _, m = toy
    n, T, lo, hi = 16, 20, c["i0"], c["i0"] + c["Lp"] - 1
    gen = torch.Generator().manual_seed(77)
    noise = [orc.draw_noise_torch(n, c["L"] * 20, 2, generator=gen) for _ in range(T)] if rng_mode == 0 else None
    for reuse in (True, False):
        out = []
        for sched in (None, (1.0, 1.0, 1.0, 1.0)):
            ch = _chains(m, c, n, T, 2, 3, rng_mode, lib, sched, 4, None, lo=lo, hi=hi, trace=True, reuse_grad=reuse)
            if rng_mode == 0:
                for U, q, u in noise:
                    ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))
            else:
                ch.run(T)
            out.append((ch.collect(), ch.trace(), ch.peek()))
            if sched is not None:
                st = ch.annealing_state()
                assert ch.annealing_shape() == (n, 3, 3) and st["events"] == 3
                assert (st["parent"] == np.arange(n)[None]).all() and (st["beta"] == 1.0).all()
                assert np.array_equal(st["ess"], np.full((3, 1), float(n))) and (st["log_mean_w"] == 0.0).all()
                assert np.array_equal(st["pre_energy"], out[-1][0]["energy_history"][[4, 8, 12]])
            ch.close()
        assert out[0][1]["accepted"].any() and not out[0][1]["accepted"].all()
        label = f"rng_mode={rng_mode} reuse={reuse}"
        _same(out[0][0], out[1][0], RESULT_KEYS, label)
        _same(out[0][1], out[1][1], ("flat", "accepted", "log_acc", "U"), label)
        _same(out[0][2], out[1][2], PEEK_KEYS, label)


# ------------------------------------------------------------------------------------------------ 2. replay
@pytest.mark.parametrize("deme", [2, 6])
@pytest.mark.parametrize("every", [1, 3])
def test_power_of_two_schedule_replays_the_reference(toy, every, deme):
    """TOY24, 12 chains, beta = (1/4, 1/2, 1), the reference fed the device's own noise and the selection uniforms restated from
    Philox: states after every iteration, accept bits, parents and the final temperatures exact; histories and pre_energy to the
    replay tolerances; pre_energy and the rewritten history row are the device's own numbers bit for bit."""
    c, lib, en, m = toy
    k = ha.REPLAY
    n, T, lo, hi = k["n"], k["T"], c["i0"], c["i0"] + c["Lp"] - 1
    ch = _chains(m, c, n, T, k["pas"], k["nmut"], 1, lib, ha.REPLAY_BETAS, every, deme, lo=lo, hi=hi, seed=k["philox_seed"],
                 trace=True, reuse_grad=False, use_graph=False)
    peeks = _stepped(ch, T)
    tr, res, st = ch.trace(), ch.collect(), ch.annealing_state()
    noise = device_noise(ch, T, k["pas"])
    ch.close()
    ref = ha.annealed_run(en, np.tile(c["wt"].astype(np.int64), (n, 1)), c["wt"], lambda t: noise[t], T, lo, hi, k["pas"], k["nmut"],
                          ha.REPLAY_BETAS, every, deme, seed=k["philox_seed"], allowed=lib)
    print(f"anneal replay every={every} D={deme}: select margin {ref['select_margin']:.3g}, replaced "
          f"{int((st['parent'] != np.arange(n)[None]).sum())} slots in {st['events']} events")
    assert ref["select_margin"] > 1e-4, "the reference's own selection sits near a tie: pick another seed"
    assert st["events"] == ha.events_cap(2, T, every) == ref["parent"].shape[0]
    for t in range(T + 1):
        assert np.array_equal(peeks[t]["idx"], ref["states"][t].numpy()), t
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(st["parent"], ref["parent"]) and np.array_equal(st["beta"], ref["beta"])
    assert (st["parent"] != np.arange(n)[None]).any(), "a replay in which nothing is ever replaced shows nothing"
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.abs(res["fitness_history"] - ref["fitness_history"].numpy()).max() <= 5e-6
    assert np.abs(st["pre_energy"] - ref["pre_energy"]).max() <= 2e-5
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy()) and np.array_equal(res["best_step"], ref["best_step"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy())
    for ev in range(st["events"]):                                           # the rewritten row: the parents' pre-selection energies
        t = (ev + 1) * every
        assert np.array_equal(res["energy_history"][t], st["pre_energy"][ev][st["parent"][ev]])
        assert np.array_equal(peeks[t]["energy"], res["energy_history"][t])


# ------------------------------------------------------------------------------------------------ 3. the plan against fp64
PLAN_BETAS = (0.5, 0.625, 0.75, 1.0)


@pytest.mark.parametrize("deme,n", [(2, 8), (6, 12), (64, 128), (70, 140), (1024, 1024)])
def test_the_plan_is_the_fp64_plan_on_the_recorded_energies(deme, n):
    """Potts only, L = 24, random start states (energies that differ from the first event on), three events, a shard that starts
    at chain 4 D: every recorded event against helpers_anneal.plan on the device's own pre_energy and the Philox uniform. parent
    equal wherever the offspring is decided (|tau_j - C_i| > 1e-9 W), at most one undecided offspring in the test; log_mean_w and
    ess within 1e-12 relative. D = 70 is no multiple of 64, D = 1024 uses four chains per thread."""
    c = hl.potts_case(24, 4, 16, seed=5)
    m = hl.hip_model_of(c)
    rng = np.random.default_rng(100 + deme)
    x0 = np.tile(c["wt"], (n, 1))
    for b in range(n):
        sites = rng.choice(np.arange(4, 20), size=rng.integers(0, 5), replace=False)
        x0[b, sites] = rng.integers(0, 20, sites.size)
    T, every, seed, off = 6, 2, 4321 + deme, 4 * deme
    ch = _chains(m, c, n, T, 2, 0, 1, None, PLAN_BETAS, every, deme, x0=x0, lo=4, hi=19, seed=seed, chain_offset=off,
                 random_chain=-1)
    ch.run(T)
    st = ch.annealing_state()
    ch.close()
    m.close()
    assert st["events"] == 3
    first = off + np.arange(n // deme) * deme
    undecided, worst_l, worst_e, replaced = 0, 0.0, 0.0, 0
    for ev in range(3):
        it = (ev + 1) * every - 1
        us = ha.select_uniforms(seed, first, it)
        db = float(np.float64(np.float32(PLAN_BETAS[ev + 1])) - np.float64(np.float32(PLAN_BETAS[ev])))
        for d in range(n // deme):
            sl = slice(d * deme, (d + 1) * deme)
            p = ha.plan(st["pre_energy"][ev, sl], db, us[d])
            loose = p["margin"] <= ha.DECIDED
            undecided += int(loose.sum())
            got = st["parent"][ev, sl] - d * deme
            if not loose.any():
                assert np.array_equal(got, p["parent"]), (ev, d)
            assert got.min() >= 0 and got.max() < deme
            replaced += int((got != np.arange(deme)).sum())
            worst_l = max(worst_l, abs(st["log_mean_w"][ev, d] - p["log_mean_w"]) / abs(p["log_mean_w"]))
            worst_e = max(worst_e, abs(st["ess"][ev, d] - p["ess"]) / p["ess"])
    print(f"anneal plan D={deme}: {replaced} slots replaced, {undecided} undecided, log_mean_w rel {worst_l:.2e}, ess rel {worst_e:.2e}")
    assert replaced > 0
    assert undecided <= 1
    assert worst_l <= 1e-12 and worst_e <= 1e-12
    assert (st["beta"] == np.float32(PLAN_BETAS[3])).all()


# ------------------------------------------------------------------------------------------------ 4. the copy
def _copy_case(name):
    import helpers_modes as hm
    from ppde_amd.energy import HipModel
    if name == "toy24":
        c, lib = hr.replay_model()
        return c, lib, hl.hip_model_of(c), 3, c["i0"], c["i0"] + c["Lp"] - 1
    if name == "toy24_potts":
        c, lib = hr.replay_model()
        return c, lib, hl.hip_model_of(c), 1, c["i0"], c["i0"] + c["Lp"] - 1
    if name in ("L104", "L237"):
        L = int(name[1:])
        c = hl.potts_case(L, {104: 23, 237: 150}[L], {104: 53, 237: 80}[L], seed=L)          # a window that does not cover the sequence
        lib = hl.seeded_library(c["wt"], c["i0"], c["i0"] + c["Lp"] - 1, seed=41)
        return c, lib, hl.hip_model_of(c), 1, 0, L - 1
    wt, J, h, cnn, st = hm.toy_parts()
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, hm.TOY["win"][0])
    m.set_cnn(cnn)
    m.set_transformer(st, hm.TOY["heads"])
    m.set_lamda(hm.LAMDA)
    c = dict(L=hm.TOY["L"], wt=wt, cnn=cnn)
    return c, hm.window_library(wt, hm.TOY["win"]), m, 7, 0, hm.TOY["L"] - 1


@pytest.mark.parametrize("name", ["toy24", "toy24_potts", "L104", "L237", "transformer"])
def test_a_replaced_slot_holds_its_parents_row(name):
    """Stepped one iteration at a time, 8 chains in demes of 4, beta = (1/4, 1/2, 1) every 2: after each event peek's row of slot d
    equals the post-accept row of parent[d], which a twin with the same seed shows whose schedule repeats the beta of that
    stage (so its selection is the identity: test 1); and the runs of both gradient policies are bit-identical, which fails when the
    gradient row or a record field is not carried."""
    c, lib, m, which, lo, hi = _copy_case(name)
    n, T, every, D, betas = 8, 6, 2, 4, (0.25, 0.5, 1.0)
    runs, replaced = {}, 0
    for reuse in (True, False):
        ch = _chains(m, c, n, T, 2, 0, 1, lib, betas, every, D, lo=lo, hi=hi, which=which, seed=515, reuse_grad=reuse, trace=True)
        peeks = _stepped(ch, T)
        runs[reuse] = (peeks, ch.collect(), ch.annealing_state(), ch.trace())
        ch.close()
    peeks, res, st, tr = runs[True]
    for t in range(T + 1):
        _same(peeks[t], runs[False][0][t], PEEK_KEYS, f"{name} t={t}")
    _same(res, runs[False][1], RESULT_KEYS, name)
    _same(st, runs[False][2], EVENT_KEYS, name)
    _same(tr, runs[False][3], ("flat", "accepted", "log_acc", "U"), name)
    assert st["events"] == 2
    for ev in range(2):
        t = (ev + 1) * every
        twin = _chains(m, c, n, T, 2, 0, 1, lib, betas[:ev + 1] + (betas[ev],), every, D, lo=lo, hi=hi, which=which, seed=515,
                       reuse_grad=True)
        twin.run(t)
        before = twin.peek()
        assert (twin.annealing_state()["parent"][ev] == np.arange(n)).all()
        twin.close()
        par = st["parent"][ev]
        assert np.array_equal(st["pre_energy"][ev], before["energy"]), (name, ev)
        for k in ("idx", "energy", "fitness", "dist"):
            assert np.array_equal(peeks[t][k], before[k][par]), (name, ev, k)
        assert np.array_equal(peeks[t]["accepted"], before["accepted"])      # the slot's own Metropolis result
        assert np.array_equal(res["random_traj"][t], before["idx"][par[0]])
        replaced += int((par != np.arange(n)).sum())
    assert (res["best_energy"] >= res["energy_history"].max(0)).all()
    print(f"anneal copy {name}: {replaced} slots replaced")
    assert replaced > 0, "a case in which nothing is replaced shows nothing"
    m.close()


# ------------------------------------------------------------------------------------------------ 5. graph replay equals eager
def test_graph_replay_equals_the_stepped_run(toy):
    """12 chains in demes of 6, 14 stages of 10 iterations: runs of 120 + 20 + 7 iterations (replays of the 100- and the
    20-segment, seven eager) against the twin stepped singly; the events behind iterations 99, 119 and 139 fall on segment ends."""
    c, lib, _, m = toy
    n, lo, hi = 12, c["i0"], c["i0"] + c["Lp"] - 1
    sched = tuple(np.linspace(0.3, 1.0, 15))
    out = []
    for graph in (True, False):
        ch = _chains(m, c, n, 147, 2, 3, 1, lib, sched, 10, 6, lo=lo, hi=hi, seed=31, use_graph=graph)
        if graph:
            for k in (120, 20, 7):
                ch.run(k)
            assert ch.graph_stats()["replayed_steps"] == 140
        else:
            for _ in range(147):
                ch.run(1)
            assert ch.graph_stats()["replayed_steps"] == 0
        out.append((ch.collect(), ch.annealing_state(), ch.peek()))
        ch.close()
    _same(out[0][0], out[1][0], RESULT_KEYS, "graph")
    _same(out[0][1], out[1][1], EVENT_KEYS, "graph")
    _same(out[0][2], out[1][2], PEEK_KEYS, "graph")
    assert out[0][1]["events"] == 14 and (out[0][1]["parent"] != np.arange(n)[None]).any()


# ------------------------------------------------------------------------------------------------ 6. the law
_KERNELS = {}
_LAW_CACHE = {}


def _kernels(name, case, betas):
    if name not in _KERNELS:
        _KERNELS[name] = (case,) + ht.kernels_of(case, betas, 2)
    return _KERNELS[name]


def _demes_against(label, m, c, betas, every, D, n_demes, T, start_rows, expected, states, index, **kw):
    S = states.shape[0]
    x0 = np.tile(np.stack([states[s].numpy().astype(np.uint8) for s in start_rows]), (n_demes, 1))
    # (room for one event even where the run ends before it: a schedule no event of which fits is refused)
    ch = _chains(m, c, n_demes * D, max(T, every), 2, c["nmut"], 1, c["allowed"], betas, every, D, x0=x0, random_chain=-1, **kw)
    ch.run(T)
    ch.sync()
    idx = ch.peek()["idx"]
    ch.close()
    cells, forbidden = ha.deme_cells(idx, D, c["allowed"], index, states[start_rows[0]].numpy(), S)
    assert forbidden == 0
    chi2, df = hl.chi_square(np.bincount(cells, minlength=S ** D).astype(np.float64), n_demes * expected)
    print(f"anneal law, {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)


@pytest.mark.parametrize("every", ha.LAW_EVERY)
def test_law_of_demes_of_two(every):
    """Case A, 2^16 demes of 2 (131 072 chains), beta = (1/2, 1): T in 1, 2, 3, 8 from the wild type and from the start state the
    CPU power test picked, against helpers_anneal.joint_law_annealed."""
    c, Ks, states, index, E, _ = _kernels("A", ht.case_a(), ha.LAW_BETAS_A)
    m = hl.hip_model_of(c)
    wt_row = index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]
    S = states.shape[0]
    for T in ha.LAW_T:
        for start in ((wt_row, wt_row), ha.POWER_START_A):
            expected = ha.joint_law_annealed(T, Ks, E, ha.LAW_BETAS_A, every, 2, start[0] * S + start[1], cache=_LAW_CACHE.setdefault("A", {}))
            _demes_against(f"case A: D=2 T={T} every={every} start={start}", m, c, ha.LAW_BETAS_A, every, 2, 1 << 16, T, start, expected,
                           states, index, seed=5977 + 13 * T + every + start[0])
    m.close()


@pytest.mark.parametrize("every", ha.LAW_EVERY)
@pytest.mark.parametrize("D", [3, 4])
def test_law_of_demes_of_three_and_four(D, every):
    """Case B, 2^15 demes, beta = (1/4, 1/2, 1): the same rows."""
    c, Ks, states, index, E, _ = _kernels("B", ht.case_b(), ha.LAW_BETAS_B)
    m = hl.hip_model_of(c)
    S = states.shape[0]
    for T in ha.LAW_T:
        for start in ((0,) * D, ha.POWER_START_B[D]):
            j0 = int(np.ravel_multi_index(start, (S,) * D))
            expected = ha.joint_law_annealed(T, Ks, E, ha.LAW_BETAS_B, every, D, j0, cache=_LAW_CACHE.setdefault(("B", D), {}))
            _demes_against(f"case B: D={D} T={T} every={every} start={start}", m, c, ha.LAW_BETAS_B, every, D, 1 << 15, T, start, expected,
                           states, index, seed=6977 + 13 * T + every + D)
    m.close()


# ------------------------------------------------------------------------------------------------ 7. the observers
def test_observers_keep_their_rules_on_the_selected_population(toy):
    """Recorder rows, site and pair counts, archive and move statistics of an annealing run (graph replay) equal their own rules
    applied to the peeks of the stepped twin without them."""
    c, lib, _, m = toy
    n, T, lo, hi, D, every = 12, 20, c["i0"], c["i0"] + c["Lp"] - 1, 6, 4
    sched = (0.25, 0.5, 0.75, 1.0)
    twin = _chains(m, c, n, T, 2, 3, 1, lib, sched, every, D, lo=lo, hi=hi, seed=77, trace=True)
    peeks = _stepped(twin, T)
    tr, res, st = twin.trace(), twin.collect(), twin.annealing_state()
    twin.close()
    sites = np.arange(lo, hi + 1, dtype=np.int32)
    ch = _chains(m, c, n, T, 2, 3, 1, lib, sched, every, D, lo=lo, hi=hi, seed=77, observers=dict(sites=sites, K=3))
    ch.run(T)
    assert ch.graph_stats()["replayed_steps"] == T
    _same(ch.collect(), res, RESULT_KEYS, "observers change nothing")
    _same(ch.annealing_state(), st, EVENT_KEYS, "observers change nothing")
    rec, (pc, ps), arc, stats = ch.recorded(), ch.pair_counts(), ch.archive(), ch.stats()
    ch.close()
    assert (st["parent"] != np.arange(n)[None]).any()
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


# ------------------------------------------------------------------------------------------------ 8. sharding and limits
def test_sharding_does_not_change_an_annealing_run(toy):
    c, lib, _, m = toy
    T, lo, hi = 12, c["i0"], c["i0"] + c["Lp"] - 1

    def run(n_, off):
        ch = _chains(m, c, n_, T, 2, 3, 1, lib, (0.25, 0.5, 1.0), 3, 4, lo=lo, hi=hi, chain_offset=off, random_chain=0 if off == 0 else -1)
        ch.run(T)
        r, st = ch.collect(), ch.annealing_state()
        ch.close()
        return r, st

    (one, st1), (a, sta), (b, stb) = run(16, 0), run(8, 0), run(8, 8)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    assert np.array_equal(np.concatenate([sta["parent"], stb["parent"] + 8], 1), st1["parent"])
    for k in ("pre_energy", "log_mean_w", "ess"):
        assert np.array_equal(np.concatenate([sta[k], stb[k]], 1), st1[k]), k
    assert np.array_equal(np.concatenate([sta["beta"], stb["beta"]]), st1["beta"])
    assert (st1["parent"] != np.arange(16)[None]).any()


def test_set_annealing_refusals_at_their_edges(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, _, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    T = 20
    ok = (0.5, 1.0)

    def fresh(n=8, **kw):
        return Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7, **kw)

    ch = fresh()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*needs reversible mode"):
        ch.set_annealing(ok, 1, 4)
    ch.set_reversible(True)
    for sched, every, deme, what in (
            (ok, 1, 1, r"2\.\.1024"), (ok, 1, 3, "n_chains must be a multiple"), (ok, 0, 4, "every must be >= 1"),
            ((1.0,), 1, 4, r"1\.\.4096"), (tuple([1.0] * 4098), 1, 4, r"1\.\.4096"), (ok, T + 1, 4, "no event would fit"),
            ((1.0, 0.5), 1, 4, "must not decrease"), ((0.0, 1.0), 1, 4, "finite and positive"), ((-1.0, 1.0), 1, 4, "finite and positive"),
            ((0.5, float("nan")), 1, 4, "finite and positive"), ((0.5, float("inf")), 1, 4, "finite and positive")):
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
            ch.set_annealing(sched, every, deme)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no annealing was set"):
        ch.annealing_shape()
    ch.set_annealing(ok, T, 2)                                                # the edges that are accepted: D = 2, one event at the very end
    ch.set_annealing(tuple([1.0] * 4097), 1, 8)                               # 4096 stages, equal neighbours
    assert ch.annealing_shape() == (8, T, 0)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set and needs reversible mode"):
        ch.set_reversible(False)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set"):
        ch.set_tempering((1.0, 0.5), 1)
    ch.set_annealing(None)
    ch.set_tempering((1.0, 0.5), 1)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*tempering is set"):
        ch.set_annealing(ok, 1, 4)
    ch.set_tempering(None)
    ch.set_reversible(False)
    ch.init(torch.as_tensor(np.tile(c["wt"], (8, 1))).cuda())
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_annealing(ok, 1, 4)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no annealing was set"):
        ch.annealing_state()
    ch.close()
    for n_, off, what in ((8, 6, "chain_offset must be a multiple"), (8, 0, None)):
        ch = fresh(n_, chain_offset=off)
        ch.set_reversible(True)
        if what:
            with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
                ch.set_annealing(ok, 1, 4)
        else:
            ch.set_annealing(ok, 1, 4)
            ch.init(torch.as_tensor(np.tile(c["wt"], (8, 1))).cuda())
            ch.run(1)
            with pytest.raises(PpdeHipError, match=r"\[-1\].*events beyond"):
                ch.annealing_state(0, 2)
            assert ch.annealing_state()["events"] == 1
        ch.close()
    ch = fresh(n_streams=2)
    ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_annealing(ok, 1, 4)
    ch.close()
    for D, fine in ((1024, True), (1025, False)):                             # the deme's upper edge
        ch = fresh(D)
        ch.set_reversible(True)
        if fine:
            ch.set_annealing(ok, 1, D)
        else:
            with pytest.raises(PpdeHipError, match=r"\[-1\].*2\.\.1024"):
                ch.set_annealing(ok, 1, D)
        ch.close()


# ------------------------------------------------------------------------------------------------ PPDE_PAS
def test_ppde_pas_runs_the_chains_a_caller_would_build_by_hand():
    import argparse
    import contextlib
    import io
    import os
    import tempfile
    from ppde_amd import synthetic
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    betas = (0.25, 0.5, 0.75, 1.0)
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True, ppde_anneal_betas=betas, ppde_anneal_every=5, ppde_deme=4)
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
        ch.set_annealing(betas, 5, 4)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res, st = ch.collect(), ch.annealing_state()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(f_hist, res["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"]) and np.array_equal(best_e, res["best_energy"])
        an = sampler.annealing
        assert an["deme"] == 4 and an["every"] == 5 and np.array_equal(an["betas"], np.asarray(betas, np.float32))
        for k in ("parent", "pre_energy", "log_mean_w", "ess"):
            assert np.array_equal(an[k], st[k]), k
        assert np.array_equal(an["beta_now"], st["beta"]) and (st["beta"] == 1.0).all() and st["events"] == 3
        assert np.array_equal(an["summary"]["log_z_ratio"], st["log_mean_w"].sum(0))
        assert "   # annealing: stage 2 of 3, beta = 0.75" in buf.getvalue() and "   # annealing: stage 3 of 3, beta = 1" in buf.getvalue()
        # the driver with the same flags: its annealing files
        import glob
        import importlib.util
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_anneal", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        res_dir = os.path.join(root, "results")
        a = drv.build_parser().parse_args([
            "--protein_weights", root, "--protein", "TOY24", "--results_path", res_dir, "--hub_dir", res_dir, "--device", "cuda:0",
            "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--n_chains", str(n), "--n_iters", str(T), "--seed", "3",
            "--log_every", "10", "--energy_lamda", "5", "--nmut_threshold", str(nmut), "--ppde_rng", "philox", "--ppde_seed", str(seed),
            "--ppde_reversible", "--ppde_anneal_betas", "0.25,0.5,0.75,1", "--ppde_anneal_every", "5", "--ppde_deme", "4",
            "--run_signature", "anneal"])
        a.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(a)
        shapes = {"anneal_parent.npy": (3, n), "anneal_pre_energy.npy": (3, n), "anneal_log_mean_w.npy": (3, 2), "anneal_ess.npy": (3, 2),
                  "anneal_betas.npy": (4,)}
        have = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
        assert set(shapes) <= have, sorted(set(shapes) - have)
        for f, shape in shapes.items():
            assert np.load(os.path.join(out, f)).shape == shape, f
        assert np.array_equal(np.load(os.path.join(out, "anneal_pre_energy.npy")), st["pre_energy"])       # the same seed: the same run
        assert np.array_equal(np.load(os.path.join(out, "anneal_parent.npy")), st["parent"])

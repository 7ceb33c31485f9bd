"""Adaptive population annealing on the GPU (ppde_chains_set_annealing_adaptive; k_select_plan_adaptive, k_select_copy): every
step is the fp64 rule of tests/helpers_anneal_adaptive.py on the device's own recorded energies, every deme of an adaptive run is
bit for bit the fixed-schedule run on its recorded beta path, graph replay equals eager issue, sharding changes nothing, the
observers keep their rules, the refusals, and PPDE_PAS and the driver.

Everything the device derives from its OWN numbers is compared bit for bit; beta_next against the numpy step to one fp32 ulp (the
rule fixes the fp64 arithmetic up to the order of the sums, which tests/test_anneal_adaptive_cpu.py shows does not reach fp32);
parent, log_mean_w and ess by tests/test_anneal_gpu.py's criteria for the plan."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_anneal as ha
import helpers_anneal_adaptive as hx
import helpers_archive as har
import helpers_library as hl
import helpers_pairs as hp
import helpers_reversible as hr
import helpers_stats as hs

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
PEEK_KEYS = ("idx", "energy", "fitness", "accepted", "dist")
EVENT_KEYS = ("parent", "pre_energy", "log_mean_w", "ess", "beta", "beta_before", "beta_after")
f32 = np.float32
STEP = 2.0 ** -12


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, adaptive=None, sched=None, every=1, deme=None, x0=None, lo=None, hi=None,
            which=None, observers=None, **kw):
    """adaptive: (beta_start, beta_end, rho, min_step[, max_stages]); sched: a fixed schedule."""
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
    if adaptive is not None:
        ch.set_annealing_adaptive(adaptive[0], adaptive[1], adaptive[2], every, deme, adaptive[4] if len(adaptive) > 4 else 4096, adaptive[3])
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


def _random_starts(c, n, seed):
    rng = np.random.default_rng(seed)
    x0 = np.tile(c["wt"], (n, 1))
    for b in range(n):
        sites = rng.choice(np.arange(4, 20), size=rng.integers(0, 5), replace=False)
        x0[b, sites] = rng.integers(0, 20, sites.size)
    return x0


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, m
    m.close()


@pytest.fixture(scope="module")
def potts24():
    c = hl.potts_case(24, 4, 16, seed=5)
    m = hl.hip_model_of(c)
    yield c, m
    m.close()


# ------------------------------------------------------------------------------------------------ 1. the step against the rule
@pytest.mark.parametrize("deme,n", [(2, 8), (6, 12), (64, 128), (70, 140), (1024, 1024)])
def test_every_step_is_the_numpy_rule_on_the_recorded_energies(potts24, deme, n):
    """Potts only, L = 24, random start states, a shard that starts at chain 4 D, every 2, four events from beta 0.25 to 1 at
    rho = 0.9 (D = 2 needs rho > 0.5: with rho <= 1 / D the first event jumps) and min_step 2^-12: beta_before is the previous
    beta_after; beta_after within one fp32 ulp of the numpy step on the device's pre_energy; the plan against helpers_anneal.plan
    with dbeta from the recorded pair (parents equal wherever decided, at most one undecided offspring, log_mean_w and ess within
    1e-12 relative). By the numpy rule alone at least one event is decided by the bisection and at least one is an arrival."""
    c, m = potts24
    T, every, seed, off, rho, start, end = 8, 2, 4321 + deme, 4 * deme, 0.9, 0.25, 1.0
    ch = _chains(m, c, n, T, 2, 0, 1, None, (start, end, rho, STEP), None, every, deme, x0=_random_starts(c, n, 100 + deme), lo=4, hi=19,
                 seed=seed, chain_offset=off, random_chain=-1)
    ch.run(T)
    st = ch.annealing_state()
    ch.close()
    assert st["events"] == 4 and st["beta_before"].shape == (4, n // deme)
    first = off + np.arange(n // deme) * deme
    kinds, undecided, worst_ulp, replaced = {}, 0, 0.0, 0
    for ev in range(4):
        us = ha.select_uniforms(seed, first, (ev + 1) * every - 1)
        assert np.array_equal(st["beta_before"][ev], st["beta_after"][ev - 1] if ev else np.full(n // deme, start, f32))
        for d in range(n // deme):
            sl = slice(d * deme, (d + 1) * deme)
            fails, rule, loose = hx.check_event(st["pre_energy"][ev, sl], st["beta_before"][ev, d], st["beta_after"][ev, d], end, rho, STEP,
                                                us[d], st["parent"][ev, sl] - d * deme, st["log_mean_w"][ev, d], st["ess"][ev, d])
            kinds[rule["by"]] = kinds.get(rule["by"], 0) + 1
            undecided += loose
            worst_ulp = max(worst_ulp, abs(float(st["beta_after"][ev, d]) - float(rule["beta_next"])) / hx.ulp32(rule["beta_next"]))
            replaced += int((st["parent"][ev, sl] - d * deme != np.arange(deme)).sum())
            assert not fails, (ev, d, fails)
    print(f"adaptive step D={deme}: {kinds}, beta_next off by at most {worst_ulp:g} ulp, {replaced} slots replaced, {undecided} undecided")
    assert kinds.get("bisect", 0) > 0, "no event of this case is decided by the bisection"
    assert kinds.get("jump", 0) + kinds.get("bisect+arrival", 0) + kinds.get("floor+arrival", 0) > 0, "no deme arrives"
    assert undecided <= 1 and replaced > 0
    assert np.array_equal(st["beta"], np.repeat(st["beta_after"][-1], deme))


# ------------------------------------------------------------------------------------------------ 2. replay as a fixed schedule
def _replay_case(name):
    if name == "potts70":
        c = hl.potts_case(24, 4, 16, seed=5)
        return c, None, hl.hip_model_of(c), 1, 4, 19, 140, 70, _random_starts(c, 140, 170), True
    c, lib = hr.replay_model()
    return c, lib, hl.hip_model_of(c), 3 if name == "toy24_cnn" else 1, c["i0"], c["i0"] + c["Lp"] - 1, 12, 6, None, False


@pytest.mark.parametrize("name,rng_mode,reuse", [("toy24", 1, True), ("toy24", 1, False), ("toy24", 0, True), ("toy24", 0, False),
                                                 ("potts70", 1, True), ("toy24_cnn", 1, True)])
def test_each_deme_replays_bit_for_bit_as_a_fixed_schedule_on_its_path(name, rng_mode, reuse):
    """An adaptive run, then for each deme k the same shape and seed under ppde_chains_set_annealing with the schedule
    (beta_start, beta_after[0..events - 1, k]): deme k's rows of both histories, the states after every event and at the end, the
    bests, parent, pre_energy, log_mean_w and ess are equal bit for bit."""
    import ppde_oracle as orc
    c, lib, m, which, lo, hi, n, D, x0, potts_only = _replay_case(name)
    T, every, pas, nmut = 8, 2, 2, 0 if potts_only else 3
    gen = torch.Generator().manual_seed(41)
    noise = [orc.draw_noise_torch(n, c["L"] * 20, pas, generator=gen) for _ in range(T)] if rng_mode == 0 else None

    def run(**mode):
        ch = _chains(m, c, n, T, pas, nmut, rng_mode, lib, every=every, deme=D, x0=x0, lo=lo, hi=hi, which=which, seed=2718,
                     reuse_grad=reuse, **mode)
        if rng_mode == 0:
            for U, q, u in noise:
                ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))
        else:
            ch.run(T)
        out = ch.collect(), ch.annealing_state(), ch.peek()
        ch.close()
        return out

    res, st, pk = run(adaptive=(0.25, 1.0, 0.9, STEP))
    assert st["events"] == 4 and (st["parent"] != np.arange(n)[None]).any()
    assert (st["beta_after"] > 0.25).all() and len({tuple(col) for col in st["beta_after"].T}) == n // D, "the demes share one path: nothing to tell apart"
    for k in range(n // D):
        sched = np.concatenate([[f32(0.25)], st["beta_after"][:, k]])
        fres, fst, fpk = run(sched=sched)
        sl = slice(k * D, (k + 1) * D)
        for key in ("energy_history", "fitness_history"):
            assert np.array_equal(res[key][:, sl], fres[key][:, sl]), (name, k, key)
        for key in ("best_idx", "best_energy", "best_fitness", "best_step"):
            assert np.array_equal(res[key][sl], fres[key][sl]), (name, k, key)
        for key in PEEK_KEYS:
            assert np.array_equal(pk[key][sl], fpk[key][sl]), (name, k, key)
        for key in ("parent", "pre_energy"):
            assert np.array_equal(st[key][:, sl], fst[key][:, sl]), (name, k, key)
        for key in ("log_mean_w", "ess", "beta_before", "beta_after"):
            assert np.array_equal(st[key][:, k], fst[key][:, k]), (name, k, key)
        assert np.array_equal(st["beta"][sl], fst["beta"][sl])
    m.close()


# ------------------------------------------------------------------------------------------------ 3. graph replay equals eager
def test_graph_replay_equals_the_stepped_run(toy):
    """12 chains in demes of 6, an event every 10 iterations: runs of 120 + 20 + 7 iterations (replays of the 100- and the
    20-segment, seven eager) against the twin stepped singly; the events behind iterations 99, 119 and 139 fall on segment ends,
    the others inside the segments."""
    c, lib, m = toy
    n, lo, hi = 12, c["i0"], c["i0"] + c["Lp"] - 1
    out = []
    for graph in (True, False):
        ch = _chains(m, c, n, 147, 2, 3, 1, lib, (0.3, 1.0, 0.97, STEP), None, 10, 6, lo=lo, hi=hi, seed=31, use_graph=graph)
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
    st = out[0][1]
    assert st["events"] == 14 and (st["parent"] != np.arange(n)[None]).any()
    assert ((st["beta_after"] > st["beta_before"]) & (st["beta_after"] < 1.0)).sum() >= 3, "the run arrives before it has chosen a step"


# ------------------------------------------------------------------------------------------------ 4. sharding
def test_sharding_does_not_change_an_adaptive_run(toy):
    c, lib, m = toy
    T, lo, hi = 12, c["i0"], c["i0"] + c["Lp"] - 1

    def run(n_, off):
        ch = _chains(m, c, n_, T, 2, 3, 1, lib, (0.25, 1.0, 0.9, STEP), None, 3, 6, lo=lo, hi=hi, chain_offset=off,
                     random_chain=0 if off == 0 else -1)
        ch.run(T)
        r, st = ch.collect(), ch.annealing_state()
        ch.close()
        return r, st

    (one, st1), (a, sta), (b, stb) = run(24, 0), run(12, 0), run(12, 12)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    assert np.array_equal(np.concatenate([sta["parent"], stb["parent"] + 12], 1), st1["parent"])
    for k in ("pre_energy", "log_mean_w", "ess", "beta_before", "beta_after"):
        assert np.array_equal(np.concatenate([sta[k], stb[k]], 1), st1[k]), k
    assert np.array_equal(np.concatenate([sta["beta"], stb["beta"]]), st1["beta"])
    assert (st1["parent"] != np.arange(24)[None]).any() and st1["events"] == 4
    assert ((st1["beta_after"] > st1["beta_before"]) & (st1["beta_after"] < 1.0)).any()


# ------------------------------------------------------------------------------------------------ 5. the observers
def test_observers_keep_their_rules_on_the_selected_population(toy):
    """Recorder rows, site and pair counts, archive and move statistics of an adaptive run (graph replay) equal their own rules
    applied to the peeks of the stepped twin without them."""
    c, lib, m = toy
    n, T, lo, hi, D, every = 12, 20, c["i0"], c["i0"] + c["Lp"] - 1, 6, 4
    mode = (0.25, 1.0, 0.9, STEP)
    twin = _chains(m, c, n, T, 2, 3, 1, lib, mode, None, every, D, lo=lo, hi=hi, seed=77, trace=True)
    peeks = _stepped(twin, T)
    tr, res, st = twin.trace(), twin.collect(), twin.annealing_state()
    twin.close()
    sites = np.arange(lo, hi + 1, dtype=np.int32)
    ch = _chains(m, c, n, T, 2, 3, 1, lib, mode, None, every, D, lo=lo, hi=hi, seed=77, observers=dict(sites=sites, K=3))
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


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_set_annealing_adaptive_refusals_at_their_edges(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    T = 20

    def fresh(n=8, **kw):
        return Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7, **kw)

    def set_(ch, start=0.25, end=1.0, rho=0.5, every=1, deme=4, stages=4096, step=STEP):
        ch.set_annealing_adaptive(start, end, rho, every, deme, stages, step)

    ch = fresh()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*needs reversible mode"):
        set_(ch)
    ch.set_reversible(True)
    below = float(np.nextafter(f32(2.0 ** -20), f32(0)))
    for kw, what in ((dict(deme=1), r"2\.\.1024"), (dict(deme=3), "n_chains must be a multiple"), (dict(every=0), "every must be >= 1"),
                     (dict(stages=0), r"max_stages must be in 1\.\.4096"), (dict(stages=4097), r"max_stages must be in 1\.\.4096"),
                     (dict(every=T + 1), "no event would fit"), (dict(start=0.0), "beta_start must be finite and positive"),
                     (dict(start=-1.0), "beta_start must be finite and positive"), (dict(start=float("nan")), "beta_start must be finite"),
                     (dict(end=float("inf")), "beta_end must be finite and positive"), (dict(end=float("nan")), "beta_end must be finite"),
                     (dict(start=1.0), "must be below beta_end"), (dict(start=1.5), "must be below beta_end"),
                     (dict(rho=0.0), r"inside \(0, 1\)"), (dict(rho=1.0), r"inside \(0, 1\)"), (dict(rho=float("nan")), r"inside \(0, 1\)"),
                     (dict(rho=-0.5), r"inside \(0, 1\)"), (dict(step=float("nan")), "min_step must be finite"),
                     (dict(step=float("inf")), "min_step must be finite"), (dict(step=below), "min_step must be finite"),
                     (dict(step=2.0 ** -19, end=2.0 + 2.0 ** -22), "min_step must be finite")):
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
            set_(ch, **kw)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no annealing was set"):
        ch.annealing_shape()
    set_(ch, step=2.0 ** -20)                                                 # the edges that are accepted: min_step at beta_end 2^-20,
    set_(ch, rho=float(np.nextafter(f32(1), f32(0))), every=T, deme=2, stages=1)   # rho just below 1, D = 2, one event at the very end
    assert ch.annealing_shape() == (2, 1, 0)
    set_(ch, rho=float(np.nextafter(f32(0), f32(1))), deme=8)                 # rho just above 0
    assert ch.annealing_shape() == (8, T, 0)
    # one mode, two forms: each replaces the other, NULL to either clears
    ch.set_annealing((0.5, 1.0), 2, 4)
    assert ch.annealing_shape() == (4, 1, 0)
    set_(ch, every=5)
    assert ch.annealing_shape() == (4, 4, 0)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set and needs reversible mode"):
        ch.set_reversible(False)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set"):
        ch.set_tempering((1.0, 0.5), 1)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*annealing is set"):
        ch.set_recombination(2, 4)
    ch.set_annealing(None)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no annealing was set"):
        ch.annealing_shape()
    ch.set_annealing((0.5, 1.0), 2, 4)
    ch.set_annealing_adaptive(None, None, None)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no annealing was set"):
        ch.annealing_shape()
    ch.set_tempering((1.0, 0.5), 1)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*tempering is set"):
        set_(ch)
    ch.set_tempering(None)
    ch.set_recombination(2, 4)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*recombination is set"):
        set_(ch)
    ch.set_recombination(0)
    set_(ch, every=2)
    ch.init(torch.as_tensor(np.tile(c["wt"], (8, 1))).cuda())
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        set_(ch)
    ch.run(3)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*events beyond"):
        ch.annealing_state(0, 2)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*ppde_chains_annealing_read_betas: events beyond"):
        ch._call("annealing_read_betas", 1, 1, None, None)
    st = ch.annealing_state()
    assert st["events"] == 1 and st["beta_before"].shape == (1, 2) and (st["beta_before"] == f32(0.25)).all()
    ch.close()
    ch = fresh(8, chain_offset=6)
    ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*chain_offset must be a multiple"):
        set_(ch)
    ch.close()
    ch = fresh(n_streams=2)
    ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        set_(ch)
    ch.close()
    for D, fine in ((1024, True), (1025, False)):                             # the deme's upper edge
        ch = fresh(D)
        ch.set_reversible(True)
        if fine:
            set_(ch, deme=D)
        else:
            with pytest.raises(PpdeHipError, match=r"\[-1\].*2\.\.1024"):
                set_(ch, deme=D)
        ch.close()


# ------------------------------------------------------------------------------------------------ 7. PPDE_PAS and the driver
def test_ppde_pas_runs_the_chains_a_caller_would_build_by_hand():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd import library as dl
    from ppde_amd import synthetic
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True, ppde_anneal_ess=0.9, ppde_anneal_beta_start=0.25,
                                  ppde_anneal_beta_end=1.0, ppde_anneal_min_step=STEP, ppde_anneal_max_stages=3, ppde_anneal_every=5,
                                  ppde_deme=4)
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
        ch.set_annealing_adaptive(0.25, 1.0, 0.9, 5, 4, 3, STEP)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res, st = ch.collect(), ch.annealing_state()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(f_hist, res["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"]) and np.array_equal(best_e, res["best_energy"])
        an = sampler.annealing
        assert an["deme"] == 4 and an["every"] == 5 and np.array_equal(an["betas"], np.array([0.25, 1.0], f32)) and st["events"] == 3
        for k in ("parent", "pre_energy", "log_mean_w", "ess"):
            assert np.array_equal(an[k], st[k]), k
        assert np.array_equal(an["beta_now"], st["beta"])
        assert an["beta_path"].shape == (4, 2) and (an["beta_path"][0] == f32(0.25)).all() and np.array_equal(an["beta_path"][1:], st["beta_after"])
        assert np.array_equal(an["summary"]["log_z_ratio"], st["log_mean_w"].sum(0))
        assert np.array_equal(an["summary"]["arrived"], st["beta_after"][-1] == 1.0)
        assert "   # annealing: stage 2, beta min / median / max = " in buf.getvalue() and " demes, min ESS = " in buf.getvalue()
        # the driver with the same flags: its annealing files
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_anneal_adaptive", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        res_dir = os.path.join(root, "results")
        a = drv.build_parser().parse_args([
            "--protein_weights", root, "--protein", "TOY24", "--results_path", res_dir, "--hub_dir", res_dir, "--device", "cuda:0",
            "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--n_chains", str(n), "--n_iters", str(T), "--seed", "3",
            "--log_every", "10", "--energy_lamda", "5", "--nmut_threshold", str(nmut), "--ppde_rng", "philox", "--ppde_seed", str(seed),
            "--ppde_reversible", "--ppde_anneal_ess", "0.9", "--ppde_anneal_beta_start", "0.25", "--ppde_anneal_min_step", str(STEP),
            "--ppde_anneal_max_stages", "3", "--ppde_anneal_every", "5", "--ppde_deme", "4", "--run_signature", "anneal_adaptive"])
        a.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(a)
        shapes = {"anneal_parent.npy": (3, n), "anneal_pre_energy.npy": (3, n), "anneal_log_mean_w.npy": (3, 2), "anneal_ess.npy": (3, 2),
                  "anneal_beta_path.npy": (4, 2)}
        have = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
        assert set(shapes) <= have and "anneal_betas.npy" not in have, sorted(have)
        for f, shape in shapes.items():
            assert np.load(os.path.join(out, f)).shape == shape, f
        path = np.load(os.path.join(out, "anneal_beta_path.npy"))
        assert (path[0] == f32(0.25)).all() and (np.diff(path, axis=0) >= 0).all()
        assert np.array_equal(np.load(os.path.join(out, "anneal_pre_energy.npy")), st["pre_energy"])       # the same seed: the same run
        assert np.array_equal(path[1:], st["beta_after"])

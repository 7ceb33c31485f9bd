"""Population annealing without a GPU: the plan of tests/helpers_anneal.py has the properties of systematic resampling, the exact
selection matrix built from it is a stochastic matrix that keeps exp(beta E)/Z moving along the schedule, `annealed_run` agrees
with that enumeration, the GPU law test of tests/test_anneal_gpu.py has the power to see the planted faults, PPDE_PAS refuses
what the mode cannot serve before it touches a device, the CLI flags parse, anneal.summarise reads a hand-made genealogy, and the
host layer runs clean under AddressSanitizer.

What each planted fault can be seen by (printed by the power test):
  sign    (weights exp(-dbeta E)) and beta (the temperature not advanced): the law rows of every case, far beyond the bound.
  reverse (the surplus list handed to the dead slots backwards): with fewer than four slots there is nothing to reverse -- one
          dead slot has one donor, two dead slots of three share one -- so only the D = 4 rows of case B see it, and the replay
          with D = 6 (parents compared exactly).
  history (row it + 1 not rewritten): the law of the STATES cannot see it by construction (expected Pearson = df exactly); the
          replay and the copy test compare the history rows and peek's energies and fail on it."""
import argparse

import numpy as np
import pytest
import torch

import helpers_anneal as ha
import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht

PAS = 2
DEMES = (2, 3, 6, 64, 70, 1024)


def _energies(rng, D, kind):
    e = rng.normal(0.0, 3.0, D).astype(np.float32)
    if kind == "ties":
        e = np.round(e)
    if kind == "nonfinite":
        e[rng.integers(0, D, max(1, D // 4))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), max(1, D // 4))
        e[rng.integers(0, D)] = 0.5                                          # (at least one finite energy)
    return e


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("D", DEMES)
def test_plan_is_systematic_resampling(D):
    """counts sum to D; n_i is floor or ceil of D w_i / W wherever the offspring are decided; survivors keep their slot; the dead
    slots take the surplus list in order; a non-finite energy is never an ancestor."""
    rng = np.random.default_rng(D)
    events = undecided = 0
    for kind in ("plain", "ties", "nonfinite"):
        for _ in range(60 if D <= 70 else 8):
            e = _energies(rng, D, kind)
            db = float(rng.choice([0.0, 0.03125, 0.25, 1.0]))
            u = float(np.float32(rng.integers(0, 1 << 24) * 2.0 ** -24))
            p = ha.plan(e, db, u)
            events += 1
            c, par = p["counts"], p["parent"]
            assert c.sum() == D and (c >= 0).all()
            fin = np.isfinite(e)
            assert (c[~fin] == 0).all() and fin[par].all()
            assert (par[c > 0] == np.flatnonzero(c > 0)).all()
            assert np.array_equal(np.sort(par), np.repeat(np.arange(D), c))
            dead = np.flatnonzero(c == 0)
            assert (np.diff(par[dead]) >= 0).all()                           # the surplus list is handed out in increasing order
            if (p["margin"] > ha.DECIDED).all():
                x = D * p["w"] / p["W"]
                assert ((c >= np.floor(x) - (x - np.floor(x) < 1e-7)) & (c <= np.ceil(x) + (np.ceil(x) - x < 1e-7))).all()
            else:
                undecided += int((p["margin"] <= ha.DECIDED).sum())
    print(f"D = {D}: {events} events, {undecided} undecided offspring at margin {ha.DECIDED} W")
    assert undecided <= 1


@pytest.mark.parametrize("D", DEMES)
def test_no_weight_change_is_the_identity_for_every_uniform(D):
    """dbeta = 0, or equal energies: the identity for every 24-bit u, the largest (1 - 2^-24) and 0 included."""
    rng = np.random.default_rng(7 * D)
    us = np.concatenate([[0.0, 1.0 - 2.0 ** -24, 2.0 ** -24, 0.5], rng.integers(0, 1 << 24, 60) * 2.0 ** -24])
    for e, db in ((_energies(rng, D, "plain"), 0.0), (np.full(D, -1.25, np.float32), 0.75), (np.zeros(D, np.float32), 2.0)):
        for u in us:
            p = ha.plan(e, db, float(np.float32(u)))
            assert np.array_equal(p["parent"], np.arange(D)) and (p["counts"] == 1).all(), (D, db, u)
            assert p["ess"] == float(D) and p["log_mean_w"] == db * float(e.max())


def test_a_deme_without_a_finite_energy_keeps_the_identity():
    p = ha.plan(np.array([np.nan, np.inf, -np.inf], np.float32), 0.5, 0.25)
    assert np.array_equal(p["parent"], np.arange(3)) and p["log_mean_w"] == -np.inf and p["ess"] == 0.0


@pytest.mark.parametrize("D", (2, 3, 6, 64))
def test_mean_offspring_over_u_is_proportional_to_the_weight(D):
    """Averaged over the 4096 uniforms k / 4096 + 2^-13 the offspring counts are D w_i / W to the grid's resolution."""
    rng = np.random.default_rng(11 * D)
    e = _energies(rng, D, "plain")
    us = (np.arange(4096) + 0.5) / 4096.0
    mean = np.mean([ha.plan(e, 0.4, u)["counts"] for u in us], 0)
    p = ha.plan(e, 0.4, 0.5)
    assert np.abs(mean - D * p["w"] / p["W"]).max() <= 2.0 / 4096.0 * 2


def test_select_uniforms_are_a_stream_of_their_own():
    """Counter (chain, it, 0x40000001, 0): neither the chain kernels' streams (0, 1, 2 + s) nor the swap's (0x40000000)."""
    import ppde_oracle as orc
    u = ha.select_uniforms(233, [0, 6], 4)
    k = np.array([233, 0], np.uint32)
    for first, got in zip((0, 6), u):
        want = (orc.philox4x32(np.array([first, 4, 0x40000001, 0], np.uint32), k)[0] >> 8) * 2.0 ** -24
        assert got == np.float32(want) and 0.0 <= got < 1.0
    assert not np.array_equal(u, ht.swap_uniforms(233, [0, 6], 4, 1)[:, 0])


# ------------------------------------------------------------------------------------------------ the exact selection matrix
@pytest.fixture(scope="module")
def case_b():
    c = ht.case_b()
    return (c,) + ht.kernels_of(c, ha.LAW_BETAS_B, PAS)


@pytest.fixture(scope="module")
def case_a():
    c = ht.case_a()
    return (c,) + ht.kernels_of(c, ha.LAW_BETAS_A, PAS)


def test_selection_matrix_is_stochastic_and_the_identity_without_a_weight_change(case_b):
    _, Ks, states, _, E, _ = case_b
    S = states.shape[0]
    for D in (2, 3):
        P = ha.selection_matrix(E, 0.25, D)
        assert P.shape == (S ** D, S ** D) and np.abs(P.sum(1) - 1.0).max() <= 1e-12 and (P >= 0).all()
        assert np.array_equal(ha.selection_matrix(E, 0.0, D), np.eye(S ** D))
        # mean offspring: the expected number of copies of letter k after selection is sum_i w_i [x_i = k] D / W
        grid = np.stack(np.unravel_index(np.arange(S ** D), (S,) * D), 1)
        x = S ** D // 3
        w = np.exp(0.25 * (np.asarray(E, np.float32).astype(np.float64)[grid[x]]))
        want = np.array([(w * (grid[x] == k)).sum() for k in range(S)]) * D / w.sum()
        got = np.array([(P[x] * (grid == k).sum(1)).sum() for k in range(S)])
        assert np.abs(got - want).max() <= 1e-9


def test_the_product_law_is_reached_along_the_schedule(case_b):
    """Started from equilibrium at beta[0] in every slot, the MARGINAL law of a slot after the schedule is close to exp(beta[S] E)/Z:
    selection of a finite deme is biased at order 1 / D (the normaliser W is random), so the distance must fall as D grows, and
    the Metropolis iterations at the new beta, which keep its law, must then drive it to zero."""
    _, Ks, states, _, E, inside = case_b
    S = states.shape[0]
    betas = np.asarray(ha.LAW_BETAS_B, np.float32).astype(np.float64)
    pi0, pi_end = hr.target_law(betas[0] * E, inside), hr.target_law(betas[-1] * E, inside)
    tvs = {}
    for D in (2, 3, 4):
        v = pi0
        for _ in range(D - 1):
            v = np.kron(v, pi0)
        P = v.copy()
        Kj = [ha.kron_power(K, D) for K in Ks]
        for s in range(2):                                                   # iteration at beta[s], then the stage to beta[s + 1]
            P = P @ Kj[s] @ ha.selection_matrix(E, float(betas[s + 1] - betas[s]), D)
        grid = np.stack(np.unravel_index(np.arange(S ** D), (S,) * D), 1)
        marg = np.array([P[grid[:, 0] == k].sum() for k in range(S)])
        tvs[D] = hr.total_variation(marg, pi_end)
        for _ in range(64):
            P = P @ Kj[2]
        assert hr.total_variation(P, ht.product_law(E, (ha.LAW_BETAS_B[-1],) * D)) <= 1e-6   # the JOINT law: the product law at beta[S]
    print("TV(slot 0 after the schedule, exp(beta_S E)/Z): " + ", ".join(f"D={D}: {t:.3e}" for D, t in tvs.items()))
    assert tvs[4] < tvs[3] < tvs[2] < hr.total_variation(pi0, pi_end)


def test_annealed_run_samples_the_enumerated_law(case_b):
    """4000 demes of 3 through `annealed_run` on explicit noise (T = 3, a stage behind every iteration) against
    joint_law_annealed, with the project's statistic and bound."""
    import ppde_oracle as orc
    c, Ks, states, index, E, _ = case_b
    S, D, T, n_demes = states.shape[0], 3, 3, 4000
    n = n_demes * D
    en = hl.oracle_energy_of(c)
    gen = torch.Generator().manual_seed(4)
    noise = [orc.draw_noise_torch(n, c["L"] * 20, PAS, generator=gen) for _ in range(T)]
    rng = np.random.default_rng(9)
    us = [rng.integers(0, 1 << 24, n_demes).astype(np.float32) * np.float32(2.0 ** -24) for _ in range(T)]
    start = (0, 3, 1)
    x0 = np.tile(np.stack([states[s].numpy() for s in start]), (n_demes, 1))
    ref = ha.annealed_run(en, x0, c["wt"], lambda t: noise[t], T, 0, c["L"] - 1, PAS, 0, ha.LAW_BETAS_B, 1, D, allowed=c["allowed"],
                          select_u=lambda it: us[it])
    cells, forbidden = ha.deme_cells(ref["final_idx"].numpy(), D, c["allowed"], index, states[start[0]].numpy(), S)
    expected = ha.joint_law_annealed(T, Ks, E, ha.LAW_BETAS_B, 1, D, int(np.ravel_multi_index(start, (S,) * D)))
    chi2, df = hl.chi_square(np.bincount(cells, minlength=S ** D).astype(np.float64), n_demes * expected)
    print(f"annealed_run against the enumeration: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert forbidden == 0 and df >= 10 and chi2 < hl.chi_square_bound(df)
    assert ref["parent"].shape == (2, n) and (ref["parent"] != np.arange(n)[None]).any() and (ref["beta"] == 1.0).all()
    for ev in range(2):                                                      # the rewritten row holds the parents' energies
        assert np.array_equal(ref["energy_history"][ev + 1].numpy(), ref["pre_energy"][ev][ref["parent"][ev]])


# ------------------------------------------------------------------------------------------------ power of the GPU law test
def _power(Ks, E, betas, D, start_joint, n):
    out, cache = {}, {}
    for fault in ha.FAULTS:
        best = (0.0, None)
        for every in ha.LAW_EVERY:
            for T in ha.LAW_T:
                p = ha.joint_law_annealed(T, Ks, E, betas, every, D, start_joint, cache=cache)
                q = ha.joint_law_annealed(T, Ks, E, betas, every, D, start_joint, fault, cache=cache)
                stat, df = ht.expected_pearson(p, q, n)
                ratio = stat / hl.chi_square_bound(df)
                if ratio > best[0]:
                    best = (ratio, (T, every, stat, df))
        out[fault] = best
    return out


def test_gpu_law_test_sees_the_planted_faults(case_a, case_b):
    """At the GPU law test's counts (2^16 demes on case A, 2^15 on case B) and from its second start state, the expected Pearson
    statistic of a run with each planted fault exceeds chi_square_bound in at least one of its rows: sign and beta in every case,
    reverse where there is something to reverse (D = 4); history leaves the states' law alone (see the module's docstring)."""
    _, KsA, stA, _, EA, _ = case_a
    _, KsB, stB, _, EB, _ = case_b
    SA, SB = stA.shape[0], stB.shape[0]
    rows = [("A", 2, _power(KsA, EA, ha.LAW_BETAS_A, 2, ha.POWER_START_A[0] * SA + ha.POWER_START_A[1], 1 << 16))]
    for D in (3, 4):
        rows.append(("B", D, _power(KsB, EB, ha.LAW_BETAS_B, D, int(np.ravel_multi_index(ha.POWER_START_B[D], (SB,) * D)), 1 << 15)))
    for case, D, pw in rows:
        for fault, (ratio, where) in pw.items():
            print(f"case {case} D={D} fault {fault}: expected Pearson / bound = {ratio:.2f} at (T, every, statistic, df) = {where}")
    for case, D, pw in rows:
        assert pw["sign"][0] > 2.0 and pw["beta"][0] > 2.0, (case, D)
        assert abs(pw["history"][0] - pw["history"][1][3] / hl.chi_square_bound(pw["history"][1][3])) < 1e-9     # blind: statistic = df
    assert rows[2][2]["reverse"][0] > 1.0
    assert rows[0][2]["reverse"][0] < 1.0 and rows[1][2]["reverse"][0] < 1.0                     # nothing to reverse below four slots


def test_replay_sees_reverse_and_history(monkeypatch):
    """The replay's reference with the surplus list reversed, or the history row left alone, differs from the right one in what the
    GPU replay compares exactly (parents, states / history rows): on the toy model's D = 6 case with the Philox noise."""
    import ppde_oracle as orc
    c, lib = hr.replay_model()
    en = hl.oracle_energy_of(c)
    k = ha.REPLAY
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    noise = [orc.device_noise(k["philox_seed"], 0, k["n"], t, k["pas"], c["L"]) for t in range(k["T"])]
    x0 = np.tile(c["wt"].astype(np.int64), (k["n"], 1))
    runs = {f: ha.annealed_run(en, x0, c["wt"], lambda t: noise[t], k["T"], lo, hi, k["pas"], k["nmut"], ha.REPLAY_BETAS, 3, 6,
                               seed=k["philox_seed"], allowed=lib, fault=f) for f in (None, "reverse", "history")}
    good = runs[None]
    print(f"replay reference every=3 D=6: select margin {good['select_margin']:.3g}, replaced {(good['parent'] != np.arange(k['n'])).sum()}")
    assert good["select_margin"] > 1e-4 and (good["parent"] != np.arange(k["n"])[None]).any()
    assert not np.array_equal(runs["history"]["energy_history"].numpy(), good["energy_history"].numpy())
    rev = runs["reverse"]
    assert not np.array_equal(rev["parent"], good["parent"]) or not np.array_equal(rev["states"].numpy(), good["states"].numpy())


# ------------------------------------------------------------------------------------------------ PPDE_PAS, CLI, summarise
class _NoDevice:
    which = 1

    def __getattr__(self, name):
        raise AssertionError(f"PPDE_PAS touched the model ({name}) before refusing")


def _args(**kw):
    return argparse.Namespace(ppde_pas_length=2, nmut_threshold=0, paper_results=False, ppde_rng="philox", seed=1, **kw)


def _x0(n):
    from ppde_amd.encoding import idx_to_onehot
    c = hl.law_case()
    return torch.from_numpy(idx_to_onehot(np.tile(c["wt"], (n, 1)))).float(), c


def test_ppde_pas_annealing_refusals_come_before_any_device_work(monkeypatch):
    from ppde_amd import sampler
    PPDE_PAS = sampler.PPDE_PAS
    s0 = PPDE_PAS(_args())
    assert s0.anneal_betas is None and s0.anneal_every == 1 and s0.deme == 0                     # off by default
    with pytest.raises(ValueError, match="ppde_reversible"):
        PPDE_PAS(_args(ppde_anneal_betas=(0.5, 1.0)))
    for bad, what in (((1.0, 0.5), "must not decrease"), ((0.0, 1.0), "positive"), ((0.5, float("nan")), "finite"),
                      ((-0.5, 1.0), "positive"), ((0.5, float("inf")), "finite"), ((1.0,), "stages"), (tuple([1.0] * 4098), "stages")):
        with pytest.raises(ValueError, match=what):
            PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=bad))
    assert PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(1.0, 1.0))).anneal_betas.size == 2   # equal neighbours are allowed
    with pytest.raises(ValueError, match="ppde_betas"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_betas=(1.0, 0.5)))
    with pytest.raises(ValueError, match="ppde_anneal_every"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_anneal_every=-1))
    for deme in (1, 1025, -2):
        with pytest.raises(ValueError, match="ppde_deme"):
            PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_deme=deme))
    with pytest.raises(ValueError, match="ppde_streams"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_streams=2))
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    x0, c = _x0(6)
    with pytest.raises(ValueError, match="no multiple of the deme of 4"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_deme=4, ppde_library=c["allowed"])).run(
            x0, 5, ef, 0, c["L"] - 1, None)
    with pytest.raises(ValueError, match="no event fits"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_anneal_every=6, ppde_library=c["allowed"])).run(
            x0, 5, ef, 0, c["L"] - 1, None)
    x1, _ = _x0(1)
    with pytest.raises(ValueError, match="2 to 1024"):                                             # deme 0 = the whole run of one chain
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_library=c["allowed"])).run(x1, 5, ef, 0, c["L"] - 1, None)
    x12, _ = _x0(12)
    s = PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_deme=4, ppde_library=c["allowed"], ppde_shard=True))
    monkeypatch.setattr(sampler, "world", lambda: (1, 2))                                        # 12 chains over 2 ranks: 6 + 6
    with pytest.raises(ValueError, match="shard boundary"):
        s.run(x12, 5, ef, 0, c["L"] - 1, None)
    monkeypatch.undo()
    # a population that fits goes on to the device (here: to the stand-in, which says so)
    with pytest.raises(AssertionError, match="touched the model"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_anneal_betas=(0.5, 1.0), ppde_deme=3, ppde_library=c["allowed"])).run(
            x0, 5, ef, 0, c["L"] - 1, None)


def test_cli_flags_parse_into_the_sampler_arguments():
    import importlib.util
    import os
    from ppde_amd.sampler import PPDE_PAS
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--ppde_anneal_betas", "0.25,0.5,1", "--ppde_anneal_every", "50", "--ppde_deme", "64",
                                       "--ppde_reversible"])
    assert a.ppde_anneal_betas == [0.25, 0.5, 1.0] and a.ppde_anneal_every == 50 and a.ppde_deme == 64
    s = PPDE_PAS(argparse.Namespace(**{**vars(a), "ppde_library": None}))
    assert np.array_equal(s.anneal_betas, np.array([0.25, 0.5, 1.0], np.float32)) and s.anneal_every == 50 and s.deme == 64
    d = mod.build_parser().parse_args([])
    assert d.ppde_anneal_betas is None and d.ppde_anneal_every == 1 and d.ppde_deme == 0
    assert PPDE_PAS(argparse.Namespace(**{**vars(d), "ppde_library": None})).anneal_betas is None


def test_summarise_reads_a_hand_made_genealogy():
    from ppde_amd import anneal
    parent, lmw, ess, want = ha.founders_by_hand()
    s = anneal.summarise(parent, lmw, ess, (0.25, 0.5, 1.0))
    assert s["deme"] == 3
    for k, v in want.items():
        assert np.array_equal(s[k], v), k
    assert s["log_z_ratio_mean"] == 0.6875 and abs(s["log_z_ratio_std"] - np.std([0.625, 0.75], ddof=1)) < 1e-15
    assert np.array_equal(s["ess_mean"], [2.25, 1.25]) and np.array_equal(s["betas"], np.array([0.25, 0.5, 1.0], np.float32))
    assert np.array_equal(anneal.compose(parent)[-1], [2, 0, 2, 3, 3, 3])
    with pytest.raises(ValueError, match="outside its slot's deme"):
        anneal.summarise(np.array([[3, 1, 2, 3, 4, 5]]), lmw[:1], ess[:1], (0.5, 1.0))
    one = anneal.summarise(np.array([[0, 0]]), np.array([[0.5]]), np.array([[1.0]]), (0.5, 1.0))        # one deme: no spread
    assert np.isnan(one["log_z_ratio_std"]) and one["founders_alive"].tolist() == [[1]]


# ------------------------------------------------------------------------------------------------ the host layer
def test_host_layer_of_annealing_under_address_sanitizer():
    """tests/hostcheck/anneal.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime of
    tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: every refusal, then create -> set_reversible -> set_annealing
    -> init -> run -> annealing_shape / read -> destroy on both RNG modes and both gradient policies, then the walk once per
    fallible runtime call with that call failing. Any leak or out-of-bounds access fails the run."""
    import os
    import re
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "anneal", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck anneal ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

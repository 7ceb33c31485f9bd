"""Adaptive population annealing without a GPU (ppde_chains_set_annealing_adaptive): the step of tests/helpers_anneal_adaptive.py
has the properties the header states, does not depend on the order of its sums at fp32 resolution, the comparison of
tests/test_anneal_adaptive_gpu.py rejects the planted faults (helpers_anneal_adaptive's docstring says which part of it sees
which), the adaptive run is the fixed-schedule run on its own beta path, PPDE_PAS refuses what the mode cannot serve before it
touches a device, the CLI flags parse, anneal.summarise reads a 2-D path, and the host layer runs clean under AddressSanitizer."""
import argparse

import numpy as np
import pytest
import torch

import helpers_anneal as ha
import helpers_anneal_adaptive as hx
import helpers_library as hl
import helpers_reversible as hr

DEMES = (2, 3, 6, 64, 70, 1024)
f32 = np.float32


def _energies(rng, D, spread, nonfinite=False):
    e = rng.normal(0.0, spread, D).astype(f32)
    if nonfinite:
        k = max(1, D // 4)
        e[rng.choice(D, k, replace=False)] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), k)
        if not np.isfinite(e).any():
            e[0] = 0.5
    return e


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("D", DEMES)
def test_step_properties(D):
    """beta_next > beta_cur and <= beta_end, arrival exact, the floor holds, and -- unless the floor or arrival decided --
    ESS(db - 2 ulp) >= target >= ESS(db + 2 ulp) with ulp the fp32 spacing at beta_next."""
    rng = np.random.default_rng(40 + D)
    end, min_step = f32(1.0), f32(2.0 ** -12)
    kinds = {}
    for trial in range(40 if D <= 70 else 6):
        spread = float(rng.choice([0.5, 3.0, 30.0, 500.0]))
        e = _energies(rng, D, spread, nonfinite=trial % 4 == 3)
        rho = f32(rng.choice([0.3, 0.5, 0.75, 0.9]))
        beta = f32(rng.choice([0.05, 0.25, 0.5, 0.9, 0.999]))
        while beta < end:
            st = hx.step(e, beta, end, rho, min_step)
            kinds[st["by"]] = kinds.get(st["by"], 0) + 1
            nxt = st["beta_next"]
            assert nxt > beta and nxt <= end and nxt.dtype == f32
            assert float(nxt) - float(beta) >= float(min_step) * (1 - 2.0 ** -20) or nxt == end
            assert st["target"] == float(rho) * int(np.isfinite(e).sum())                  # rho F, not rho D
            if st["by"] == "bisect":
                u, db = hx.ulp32(nxt), st["db"]
                assert hx.ess_of(st["x"], db - 2 * u) >= st["target"] >= hx.ess_of(st["x"], db + 2 * u), (D, trial, float(beta))
            if "arrival" in st["by"] or st["by"] == "jump":
                assert nxt == end                                                          # exact
            beta = nxt
            e = _energies(rng, D, spread, nonfinite=trial % 4 == 3)
        assert hx.step(e, end, end, rho, min_step)["by"] == "arrived" and hx.step(e, end, end, rho, min_step)["db"] == 0.0
    print(f"D = {D}: {kinds}")
    assert kinds.get("bisect", 0) > 0 and kinds.get("jump", 0) > 0           # (the floor: test_min_step_floor_moves_a_collapsed_deme)


@pytest.mark.parametrize("D", DEMES)
def test_equal_energies_and_small_targets_jump(D):
    """All energies equal: ESS = F at every d, the deme jumps to beta_end. rho <= 1 / D: ESS >= 1 >= rho D always, the first event
    jumps whatever the energies (D = 2 with rho = 0.5 always jumps). Without a finite energy beta stays."""
    rng = np.random.default_rng(90 + D)
    st = hx.step(np.full(D, -3.25, f32), 0.125, 1.0, 0.99, 2.0 ** -12)
    assert st["beta_next"] == f32(1.0) and st["by"] == "jump" and st["db"] == 0.875
    for spread in (0.5, 30.0, 500.0):
        st = hx.step(_energies(rng, D, spread), 0.125, 1.0, f32(1.0 / D) * (1 - 2.0 ** -23), 2.0 ** -12)
        assert st["beta_next"] == f32(1.0) and st["by"] == "jump", (D, spread)
    st = hx.step(np.array([np.nan, np.inf] * (D // 2) + [-np.inf] * (D % 2), f32), 0.125, 1.0, 0.5, 2.0 ** -12)
    assert st["beta_next"] == f32(0.125) and st["by"] == "empty" and st["db"] == 0.0


def test_nonfinite_energies_use_rho_F():
    """Four finite energies of six at rho = 0.7: the target is 2.8, not 4.2 -- with two equal maxima and the rest far below,
    ESS falls to 2 at a small d, so rho D = 4.2 would stop far earlier than rho F = 2.8 does."""
    e = np.array([1.0, np.nan, 1.0, -2.0, np.inf, -2.5], f32)
    good, bad = hx.step(e, 0.1, 4.0, 0.7, 2.0 ** -12), hx.step(e, 0.1, 4.0, 0.7, 2.0 ** -12, fault="target_D")
    assert good["F"] == 4 and good["target"] == float(f32(0.7)) * 4 and bad["target"] == float(f32(0.7)) * 6
    assert bad["by"] == "floor" and good["by"] == "bisect" and good["beta_next"] > bad["beta_next"]   # (ESS <= F = 4 < 4.2 at any d)


def test_min_step_floor_moves_a_collapsed_deme():
    """One energy far above the rest: ESS falls below the target at any representable step, the floor is what moves the deme, and
    (beta_end - beta_start) / min_step bounds the stages."""
    e = np.array([5000.0] + [0.0] * 63, f32)
    beta, stages = f32(0.25), 0
    while beta < 1.0:
        st = hx.step(e, beta, 1.0, 0.9, 2.0 ** -4)
        assert "floor" in st["by"] and (st["beta_next"] == f32(float(beta) + 2.0 ** -4) or st["beta_next"] == f32(1.0))
        beta = st["beta_next"]
        stages += 1
    assert stages == 12


def test_summation_order_does_not_move_beta_next():
    """Random energies at D in {2, 6, 64, 70, 1024}, spreads 0.5 to 500, from beta = 0.05 to 1 at rho = 0.5 and min_step 2^-12,
    each step evaluated with three orders of summation (numpy's pairwise, forward, backward): the same fp32 beta_next. (A reduced
    form of the 35 612-step check made when the rule was written, which found no difference either.)"""
    rng = np.random.default_rng(2024)
    steps = differ = 0
    for D in (2, 6, 64, 70, 1024):
        for spread in (0.5, 5.0, 50.0, 500.0):
            for _ in range(6 if D < 1024 else 2):
                beta = f32(0.05)
                while beta < 1.0:
                    e = _energies(rng, D, spread)
                    got = [hx.step(e, beta, 1.0, 0.5, 2.0 ** -12, order=o)["beta_next"] for o in hx.ORDERS]
                    steps += 1
                    differ += int(len(set(float(g) for g in got)) > 1)
                    beta = got[0]
    print(f"{steps} steps, {differ} with a beta_next that depends on the order of summation")
    assert steps > 1000 and differ == 0


# ------------------------------------------------------------------------------------------------ planted faults
def _device_like(e, beta, end, rho, min_step, u, fault):
    """What a device with the planted fault would record for one event of one deme."""
    st = hx.step(e, beta, end, rho, min_step, fault=fault)
    p = ha.plan(e, st["db"], u)
    return st["beta_next"], p["parent"], p["log_mean_w"], p["ess"]


def test_every_planted_fault_is_rejected_by_the_gpu_comparison():
    """helpers_anneal_adaptive.check_event -- the comparison of the GPU step test -- passes the right step on every case and fails
    each planted fault on at least one; which part fails is printed and stated in helpers_anneal_adaptive's docstring. 'hi' with all
    48 halvings cannot be seen by ANY fp32 comparison (the bracket is 2^-48 dmax wide): that is asserted too, and the fault is
    planted with 8 halvings in its place."""
    rng = np.random.default_rng(31)
    end, min_step = f32(1.0), f32(2.0 ** -12)
    cases = []
    for D in (6, 64, 70):
        for spread in (3.0, 30.0, 500.0, 5000.0):
            for nonfinite in (False, True):
                cases.append((_energies(rng, D, spread, nonfinite), f32(rng.choice([0.05, 0.25, 0.5])), f32(rng.choice([0.5, 0.75, 0.9])),
                              float(f32(rng.integers(0, 1 << 24) * 2.0 ** -24))))
        # (energies far from 0 with a small spread: unshifted, exp overflows where the shifted rule takes a large step)
        cases.append((_energies(rng, D, 0.5) + f32(2000.0), f32(0.25), f32(0.5), 0.375))
    seen = {f: set() for f in (None,) + hx.FAULTS}
    for fault in seen:
        for e, beta, rho, u in cases:
            b, par, lmw, ess = _device_like(e, beta, end, rho, min_step, u, fault)
            fails, _, loose = hx.check_event(e, beta, b, end, rho, min_step, u, par, lmw, ess)
            seen[fault].update(f.split()[0] for f in fails)
    print({str(k): sorted(v) for k, v in seen.items()})
    assert not seen[None]
    for fault in ("target_D", "no_shift", "hi8", "no_floor"):
        assert "beta_next" in seen[fault], fault
    assert "beta_next" not in seen["delta_w"] and {"log_mean_w", "ess"} & seen["delta_w"]
    for e, beta, rho, u in cases:                                            # lo and hi after 48 halvings: one fp32 number
        st = hx.step(e, beta, end, rho, min_step)
        if st["by"] == "bisect":
            assert abs(float(f32(float(beta) + st["delta"] + st["dmax"] * 2.0 ** -48)) - float(st["beta_next"])) <= hx.ulp32(st["beta_next"])


def test_adaptive_run_is_the_fixed_run_on_its_own_path_and_the_replay_sees_delta_w():
    """TOY24, one deme of 6, every 3, device noise restated from Philox: helpers_anneal.annealed_run on the adaptive run's beta path
    gives the adaptive run's arrays exactly; with the resampling weights taken from d instead of the rounded beta pair the path is
    the same to the first event and the events' log_mean_w differ -- which is what the GPU's fixed-schedule replay compares bit for
    bit."""
    import ppde_oracle as orc
    c, lib = hr.replay_model()
    en = hl.oracle_energy_of(c)
    k = ha.REPLAY
    D, T, every = 6, 9, 3
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    noise = [orc.device_noise(k["philox_seed"], 0, D, t, k["pas"], c["L"]) for t in range(T)]
    x0 = np.tile(c["wt"].astype(np.int64), (D, 1))
    kw = dict(seed=k["philox_seed"], allowed=lib)
    runs = {f: hx.adaptive_run(en, x0, c["wt"], lambda t: noise[t], T, lo, hi, k["pas"], k["nmut"], 0.25, 1.0, 0.8, 2.0 ** -12, every, D,
                               fault=f, **kw) for f in (None, "delta_w")}
    good = runs[None]
    path = good["beta_path"]
    print(f"adaptive reference: path {path.tolist()}, replaced {(good['parent'] != np.arange(D)).sum()}")
    assert path[0] == f32(0.25) and (np.diff(path) >= 0).all() and path.size == 4 and (path[1:] > path[0]).all()
    fixed = ha.annealed_run(en, x0, c["wt"], lambda t: noise[t], T, lo, hi, k["pas"], k["nmut"], path, every, D, **kw)
    for key in ("parent", "pre_energy", "log_mean_w", "ess", "beta"):
        assert np.array_equal(good[key], fixed[key]), key
    assert torch.equal(good["states"], fixed["states"]) and torch.equal(good["energy_history"], fixed["energy_history"])
    bad = runs["delta_w"]
    assert bad["beta_path"][1] == path[1]
    if 0.25 < float(path[1]) < 1.0 and float(path[1]) - 0.25 != hx.step(good["pre_energy"][0], 0.25, 1.0, 0.8, 2.0 ** -12)["delta"]:
        assert bad["log_mean_w"][0, 0] != fixed["log_mean_w"][0, 0]


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


def test_ppde_pas_adaptive_refusals_come_before_any_device_work():
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(_args()).anneal_adaptive is None                                              # off by default
    ok = dict(ppde_reversible=True, ppde_anneal_ess=0.5, ppde_anneal_beta_start=0.25)
    s = PPDE_PAS(_args(**ok))
    assert s.anneal_adaptive == dict(ess_target=0.5, beta_start=0.25, beta_end=1.0, min_step=float(f32(0.75 / 4096)), max_stages=4096)
    assert s.anneal_betas is None
    for bad, what in ((dict(ppde_reversible=False), "ppde_reversible"), (dict(ppde_anneal_betas=(0.5, 1.0)), "cannot be combined"),
                      (dict(ppde_betas=(1.0, 0.5)), "ppde_betas"), (dict(ppde_anneal_beta_start=None), "ppde_anneal_beta_start"),
                      (dict(ppde_anneal_ess=0.0), r"\(0, 1\)"), (dict(ppde_anneal_ess=1.0), r"\(0, 1\)"),
                      (dict(ppde_anneal_ess=float("nan")), r"\(0, 1\)"), (dict(ppde_anneal_beta_start=0.0), "finite and positive"),
                      (dict(ppde_anneal_beta_end=float("inf")), "finite and positive"), (dict(ppde_anneal_beta_start=1.0), "below"),
                      (dict(ppde_anneal_beta_start=2.0), "below"), (dict(ppde_anneal_min_step=float("nan")), "ppde_anneal_min_step"),
                      (dict(ppde_anneal_min_step=2.0 ** -21), "ppde_anneal_min_step"), (dict(ppde_anneal_max_stages=0), "1..4096"),
                      (dict(ppde_anneal_max_stages=4097), "1..4096"), (dict(ppde_anneal_every=0, ppde_anneal_betas=None), None),
                      (dict(ppde_anneal_every=-1), "ppde_anneal_every"), (dict(ppde_deme=1), "ppde_deme"),
                      (dict(ppde_deme=1025), "ppde_deme"), (dict(ppde_streams=2), "ppde_streams"),
                      (dict(ppde_recombine_every=2), "ppde_recombine_every")):
        if what is None:                                                                          # (every 0 reads as the default 1, as for a schedule)
            assert PPDE_PAS(_args(**{**ok, **bad})).anneal_every == 1
            continue
        with pytest.raises(ValueError, match=what):
            PPDE_PAS(_args(**{**ok, **bad}))
    assert PPDE_PAS(_args(**{**ok, "ppde_anneal_min_step": 2.0 ** -20})).anneal_adaptive["min_step"] == 2.0 ** -20   # the edge
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    x0, c = _x0(6)
    with pytest.raises(ValueError, match="no multiple of the deme of 4"):
        PPDE_PAS(_args(**ok, ppde_deme=4, ppde_library=c["allowed"])).run(x0, 5, ef, 0, c["L"] - 1, None)
    with pytest.raises(ValueError, match="no event fits"):
        PPDE_PAS(_args(**ok, ppde_anneal_every=6, ppde_library=c["allowed"])).run(x0, 5, ef, 0, c["L"] - 1, None)
    with pytest.raises(AssertionError, match="touched the model"):
        PPDE_PAS(_args(**ok, ppde_deme=3, ppde_library=c["allowed"])).run(x0, 5, ef, 0, c["L"] - 1, None)


def test_cli_flags_parse_into_the_sampler_arguments():
    import importlib.util
    import os
    from ppde_amd.sampler import PPDE_PAS
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli_adaptive", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--ppde_anneal_ess", "0.6", "--ppde_anneal_beta_start", "0.125", "--ppde_anneal_beta_end", "2",
                                       "--ppde_anneal_min_step", "0.01", "--ppde_anneal_max_stages", "300", "--ppde_anneal_every", "50",
                                       "--ppde_deme", "64", "--ppde_reversible"])
    s = PPDE_PAS(argparse.Namespace(**{**vars(a), "ppde_library": None}))
    assert s.anneal_adaptive == dict(ess_target=float(f32(0.6)), beta_start=0.125, beta_end=2.0, min_step=float(f32(0.01)), max_stages=300)
    assert s.anneal_every == 50 and s.deme == 64 and s.anneal_betas is None
    d = mod.build_parser().parse_args([])
    assert d.ppde_anneal_ess is None and d.ppde_anneal_beta_start is None and d.ppde_anneal_beta_end == 1.0
    assert d.ppde_anneal_min_step is None and d.ppde_anneal_max_stages == 4096
    assert PPDE_PAS(argparse.Namespace(**{**vars(d), "ppde_library": None})).anneal_adaptive is None


def test_summarise_reads_a_two_dimensional_path():
    from ppde_amd import anneal
    parent, lmw, ess, want = ha.founders_by_hand()
    path = np.array([[0.25, 0.25], [0.5, 1.0], [0.75, 1.0]], f32)                # deme 1 arrives at the first event, deme 0 never
    s = anneal.summarise(parent, lmw, ess, path, beta_end=1.0)
    assert np.array_equal(s["arrived"], [False, True]) and np.array_equal(s["stages"], [-1, 1])
    assert s["log_z_ratio_mean"] == want["log_z_ratio"][1] and np.isnan(s["log_z_ratio_std"])
    assert np.array_equal(s["log_z_ratio"], want["log_z_ratio"]) and np.array_equal(s["founders_alive"], want["founders_alive"])
    assert np.array_equal(s["replaced"], want["replaced"]) and np.array_equal(s["betas"], path)
    both = anneal.summarise(parent, lmw, ess, np.array([[0.25, 0.25], [0.5, 1.0], [1.0, 1.0]], f32))      # (beta_end: the path's maximum)
    assert both["arrived"].all() and np.array_equal(both["stages"], [2, 1])
    assert both["log_z_ratio_mean"] == want["log_z_ratio"].mean() and both["log_z_ratio_std"] == want["log_z_ratio"].std(ddof=1)
    none = anneal.summarise(parent, lmw, ess, path[:, :1].repeat(2, 1), beta_end=1.0)
    assert not none["arrived"].any() and np.isnan(none["log_z_ratio_mean"]) and (none["stages"] == -1).all()
    one = anneal.summarise(parent, lmw, ess, (0.25, 0.5, 1.0))                    # 1-D: what it gave before
    assert "arrived" not in one and np.array_equal(one["betas"], np.array([0.25, 0.5, 1.0], f32))
    with pytest.raises(ValueError, match="columns"):
        anneal.summarise(parent, lmw, ess, np.ones((3, 3), f32))


def test_host_layer_of_adaptive_annealing_under_address_sanitizer():
    """tests/hostcheck/anneal_adaptive.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock
    runtime of tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: every refusal, then set -> shape -> init -> run ->
    both reads -> clear, replacement by the fixed form and back, then the walk once per fallible runtime call with that call
    failing. Any leak or out-of-bounds access fails the run."""
    import os
    import re
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "anneal_adaptive", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck anneal_adaptive ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

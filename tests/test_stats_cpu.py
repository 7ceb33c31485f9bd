"""The move statistics without a GPU: the rule (helpers_stats.stats_of) on hand-made peeks, its identities on random inputs,
ppde_amd.stats.summarise, what PPDE_PAS refuses before any device work, the driver's flags, the host side of the C ABI as a
stand-alone program under AddressSanitizer (tests/hostcheck/stats.cpp), and the conditions the GPU tests of tests/test_stats_gpu.py
stand on, asserted on CPU reference runs of the same configurations (TOY24, 16 chains, T = 130, pas_length 2, nmut_threshold 3,
Philox seed 202). The tests assert ">= 1" of each kind of event, not the counts they print."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_reversible as hr
import helpers_stats as hs
import helpers_tempering as ht

WT = np.array([3, 3, 3, 3], np.uint8)


def _peeks(rows):
    """Peeks of a population from a list of [n, L] letter arrays: dist from the wild type WT."""
    return [dict(idx=np.asarray(r, np.uint8), dist=(np.asarray(r, np.uint8) != WT[None]).sum(1).astype(np.int32)) for r in rows]


# ------------------------------------------------------------------------------------------------ the rule on hand-made peeks
def test_an_accepted_iteration_whose_state_did_not_change_counts_as_accepted_not_as_moved():
    x = [[3, 5, 3, 3]]
    st = hs.stats_of(_peeks([x, x, [[3, 5, 7, 3]]]), [[1], [1]], [[2], [3]], mu_max=3)
    assert st["iters"].tolist() == [[2]] and st["accepts"].tolist() == [[2]] and st["moved"].tolist() == [[1]]
    assert st["jump_sum"].tolist() == [[1]] and st["dist_sum"].tolist() == [[1 + 2]] and st["wt_returns"].tolist() == [[0]]
    assert st["len_attempts"].tolist() == [[0, 1, 1]] and st["len_accepts"].tolist() == [[0, 1, 1]]
    assert st["site_changes"].tolist() == [[0, 0, 1, 0]]
    hs.assert_identities(st, 2)


def test_a_return_to_the_wild_type_is_counted_once_and_only_from_a_mutant():
    rows = [[[3, 3, 3, 3]], [[3, 9, 3, 3]], [[3, 3, 3, 3]], [[3, 3, 3, 3]], [[1, 2, 3, 3]], [[3, 3, 3, 3]]]
    st = hs.stats_of(_peeks(rows), [[1], [1], [0], [1], [1]], [[1], [1], [1], [2], [3]], mu_max=3)
    assert st["wt_returns"].tolist() == [[2]] and st["moved"].tolist() == [[4]] and st["jump_sum"].tolist() == [[1 + 1 + 0 + 2 + 2]]
    assert st["dist_sum"].tolist() == [[1 + 0 + 0 + 2 + 0]] and st["accepts"].tolist() == [[4]]
    assert st["len_attempts"].tolist() == [[3, 1, 1]] and st["len_accepts"].tolist() == [[2, 1, 1]]
    assert st["site_changes"].tolist() == [[2, 4, 0, 0]]
    hs.assert_identities(st, 5)


def test_an_iteration_belongs_to_the_rung_it_ran_on_not_the_one_the_swap_left():
    rows = [[[3, 3, 3, 3], [3, 3, 3, 3]], [[4, 3, 3, 3], [3, 3, 3, 3]], [[4, 3, 3, 3], [3, 3, 3, 8]]]
    hist = np.array([[0, 1], [1, 0], [1, 0]], np.uint8)            # the swap of iteration 0 exchanged the two chains' rungs
    st = hs.stats_of(_peeks(rows), [[1, 0], [0, 1]], [[1, 2], [3, 1]], hist, 2, 3)
    assert st["iters"].tolist() == [[1, 1], [1, 1]]
    assert st["accepts"].tolist() == [[1, 0], [1, 0]]               # chain 0 accepted on rung 0, chain 1 (later) on rung 0 too
    assert st["jump_sum"].tolist() == [[1, 0], [1, 0]]
    assert st["len_attempts"].tolist() == [[2, 0, 0], [0, 1, 1]] and st["len_accepts"].tolist() == [[2, 0, 0], [0, 0, 0]]
    assert st["site_changes"].tolist() == [[1, 0, 0, 1], [0, 0, 0, 0]]
    hs.assert_identities(st, 2)
    ev = hs.events(_peeks(rows), [[1, 0], [0, 1]], [[1, 2], [3, 1]], hist, 2, 3)
    assert ev["rung_moves"] == 2 and ev["changed_sites"].tolist() == [0, 3]


@pytest.mark.parametrize("seed", range(4))
def test_the_identities_hold_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    n, L, T, R, M = 7, 9, 40, 3, 5
    wt = rng.integers(0, 20, L).astype(np.uint8)
    rows, x = [], np.tile(wt, (n, 1))
    acc, U, hist = rng.integers(0, 2, (T, n)), rng.integers(1, M + 1, (T, n)), rng.integers(0, R, (T + 1, n)).astype(np.uint8)
    rows.append(x.copy())
    for t in range(T):
        for b in np.flatnonzero(acc[t]):                            # an accepted chain moves along up to U residues, or not at all
            for l in rng.integers(0, L, rng.integers(0, U[t, b] + 1)):
                x[b, l] = rng.integers(0, 3) + wt[l] * (rng.random() < 0.5)
        rows.append(x.copy() % 20)
        x = rows[-1].copy()
    peeks = [dict(idx=r, dist=(r != wt[None]).sum(1)) for r in rows]
    st = hs.stats_of(peeks, acc, U, hist, R, M)
    hs.assert_identities(st, T)
    assert st["iters"].sum() == n * T and st["accepts"].sum() == acc.sum()
    # the sums over the ranks of a split population are the unsplit ones, and the per-chain rows are the unsplit rows
    a = hs.stats_of([dict(idx=p["idx"][:3], dist=p["dist"][:3]) for p in peeks], acc[:, :3], U[:, :3], hist[:, :3], R, M)
    b = hs.stats_of([dict(idx=p["idx"][3:], dist=p["dist"][3:]) for p in peeks], acc[:, 3:], U[:, 3:], hist[:, 3:], R, M)
    for k in hs.PER_CHAIN:
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), st[k]), k
    for k in ("len_attempts", "len_accepts", "site_changes"):
        assert np.array_equal(a[k] + b[k], st[k]), k
    from ppde_amd.stats import summarise
    whole = summarise(st)
    joined = {k: np.concatenate([a[k], b[k]], 0) for k in hs.PER_CHAIN}
    joined.update({k: a[k] + b[k] for k in ("len_attempts", "len_accepts", "site_changes")})
    for k, v in summarise(joined).items():
        assert v is None or np.array_equal(np.asarray(v), np.asarray(whole[k]), equal_nan=True), k


# ------------------------------------------------------------------------------------------------ summarise
def test_summarise_on_hand_made_counters():
    from ppde_amd import stats
    assert stats.KEYS == hs.KEYS
    raw = dict(iters=np.array([[10, 0], [6, 4]]), accepts=np.array([[5, 0], [3, 1]]), moved=np.array([[4, 0], [3, 1]]),
               jump_sum=np.array([[6, 0], [4, 2]]), dist_sum=np.array([[20, 0], [12, 2]]), wt_returns=np.array([[1, 0], [0, 1]]),
               len_attempts=np.array([[8, 8, 0], [2, 2, 0]]), len_accepts=np.array([[6, 2, 0], [1, 0, 0]]),
               site_changes=np.array([[8, 2, 0], [0, 2, 0]]))
    s = stats.summarise(raw, betas=[1.0, 0.5])
    assert s["acceptance"] == 9 / 20
    assert np.allclose(s["acceptance_by_rung"], [8 / 16, 1 / 4]) and np.allclose(s["acceptance_by_chain"], [0.5, 0.4])
    assert np.allclose(s["acceptance_by_length"][:, :2], [[0.75, 0.25], [0.5, 0.0]]) and np.isnan(s["acceptance_by_length"][:, 2]).all()
    assert np.allclose(s["mean_jump"], [10 / 8, 2 / 1]) and np.allclose(s["moved_fraction"], [7 / 16, 1 / 4])
    assert np.allclose(s["mean_dist"], [32 / 16, 2 / 4]) and np.allclose(s["wt_returns_per_1000"], [1000 / 16, 1000 / 4])
    assert np.allclose(s["site_mobility"], [[8 / 16, 2 / 16, 0], [0, 2 / 4, 0]]) and s["betas"].tolist() == [1.0, 0.5]
    s = stats.summarise(dict(raw, site_changes=None))
    assert s["site_mobility"] is None and s["betas"] is None
    empty = stats.summarise({k: np.zeros_like(v) for k, v in raw.items()})                       # nothing ran: nan, not an error
    assert np.isnan(empty["acceptance"]) and np.isnan(empty["acceptance_by_rung"]).all() and np.isnan(empty["site_mobility"]).all()
    assert stats.log_line(raw) == "   # acceptance so far = 0.450 (path length 1: 0.70, 2: 0.20)"


# ------------------------------------------------------------------------------------------------ PPDE_PAS and the driver
def _args(**kw):
    base = dict(ppde_pas_length=2, nmut_threshold=0, paper_results=False, ppde_rng="philox", seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_ppde_pas_stats_spellings_and_refusals_come_before_any_device_work():
    from ppde_amd.sampler import PPDE_PAS, check_stats
    assert PPDE_PAS(_args()).stats_spec is None and PPDE_PAS(_args()).stats is None               # off by default
    for off in (None, False):
        assert PPDE_PAS(_args(ppde_stats=off)).stats_spec is None
    assert PPDE_PAS(_args(ppde_stats=True)).stats_spec is True
    assert PPDE_PAS(_args(ppde_stats="no-sites")).stats_spec == "no-sites"
    assert PPDE_PAS(_args(ppde_stats=True, paper_results=True)).stats_spec is True               # paper_results is counted too
    for bad in (1, 0, "yes", "sites", 2.5, []):
        with pytest.raises(ValueError, match="ppde_stats.*no-sites"):
            PPDE_PAS(_args(ppde_stats=bad))
    with pytest.raises(ValueError, match="ppde_stats.*ppde_streams"):
        PPDE_PAS(_args(ppde_stats=True, ppde_streams=2))
    assert check_stats(None, 2) is None and PPDE_PAS(_args(ppde_streams=2)).stats_spec is None   # ... which alone stays what it was


def test_cli_flags_parse_into_the_sampler_argument():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli_stats", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = mod.build_parser().parse_args([])
    assert d.ppde_stats is False and d.ppde_stats_no_sites is False
    assert mod.get_sampler(d).stats_spec is None                                                 # the defaults switch nothing on
    assert mod.get_sampler(mod.build_parser().parse_args(["--ppde_stats"])).stats_spec is True
    assert mod.get_sampler(mod.build_parser().parse_args(["--ppde_stats_no_sites"])).stats_spec == "no-sites"
    assert mod.get_sampler(mod.build_parser().parse_args(["--ppde_stats", "--ppde_stats_no_sites"])).stats_spec == "no-sites"


# ------------------------------------------------------------------------------------------------ the host layer
def test_host_layer_of_the_statistics_under_address_sanitizer():
    """tests/hostcheck/stats.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime of
    tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: set, replace and clear, every refusal, reads before and after
    runs, a second init and destroy, then the walk once per fallible runtime call with that call failing. Any leak or out-of-bounds
    access fails the run."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "stats", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck stats ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ what the GPU tests stand on
N, T, PAS, NMUT, SEED = 16, 130, 2, 3, 202


def _reference(mode, swap_every=1):
    """The oracle iteration of a mode on the toy configuration of tests/test_stats_gpu.py, fed the device RNG's draws."""
    import ppde_oracle as orc
    c, lib = hr.replay_model()
    en = hl.oracle_energy_of(c)
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    x0 = np.tile(c["wt"].astype(np.int64), (N, 1))
    draws = [orc.device_noise(SEED, 0, N, t, PAS, c["L"]) for t in range(T)]

    def noise(t):
        return draws[t]

    if mode == "default":
        r = orc.run(en, x0, c["wt"], noise, T, lo, hi, PAS, NMUT, record_after_reset=True)       # (states as peek shows them)
    elif mode == "library":
        r = hl.masked_run(lib, en, x0, c["wt"], noise, T, lo, hi, PAS, NMUT, record_after_reset=True)
    elif mode == "reversible":
        r = hr.reversible_run(en, x0, c["wt"], noise, T, lo, hi, PAS, NMUT, allowed=lib)
    else:
        r = ht.tempered_run(en, x0, c["wt"], noise, T, lo, hi, PAS, NMUT, ht.REPLAY_BETAS, swap_every, seed=SEED, allowed=lib)
    states = r["states"].numpy().astype(np.uint8)
    peeks = [dict(idx=states[t], dist=(states[t] != c["wt"][None]).sum(1)) for t in range(T + 1)]
    U = np.stack([np.asarray(d[0]).reshape(-1) for d in draws]).clip(1, 2 * PAS - 1)
    hist, R = (r["rung_history"], len(ht.REPLAY_BETAS)) if mode == "tempering" else (None, 0)
    return c, lib, peeks, r["accepted"].numpy(), U, hist, R


@pytest.mark.parametrize("mode,swap_every", [("default", 1), ("library", 1), ("reversible", 1), ("tempering", 1), ("tempering", 3)])
def test_the_toy_configurations_take_every_branch_the_gpu_tests_rely_on(mode, swap_every):
    c, lib, peeks, acc, U, hist, R = _reference(mode, swap_every)
    ev = hs.events(peeks, acc, U, hist, R, 2 * PAS - 1)
    print(f"TOY24 {mode} swap_every={swap_every}: {ev}")
    assert (ev["acc_by_len"] >= 1).all() and (ev["rej_by_len"] >= 1).all()                       # both outcomes at every path length 1..3
    assert ev["short_jumps"] + ev["still_accepts"] >= 1                                          # an accepted iteration with h < U
    assert ev["moved_without_accept"] == 0
    if mode == "default":
        assert ev["wt_returns"] >= 1                                                            # the cap resets to the wild type
    if mode == "tempering":
        assert ev["rung_moves"] >= 1                                                            # a rung after the swap that was not iterated on
    if mode != "default":
        lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
        is_open = np.flatnonzero(np.asarray(lib)[lo:hi + 1] != 0) + lo
        assert np.array_equal(ev["changed_sites"], is_open), (ev["changed_sites"], is_open)      # every open residue, no frozen one
    st = hs.stats_of(peeks, acc, U, hist, R, 2 * PAS - 1)
    hs.assert_identities(st, T)
    assert (U[1:] != U[:-1]).any()

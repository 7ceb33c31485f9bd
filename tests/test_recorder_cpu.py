"""The recorder without a GPU: the row schedule at its edges, what PPDE_PAS refuses before any device work, the host side of the
C ABI as a stand-alone program under AddressSanitizer (tests/hostcheck/recorder.cpp), and the conditions the GPU law tests of
tests/test_recorder_gpu.py stand on.

Enumerated here (CPU, fp64 over the reference's fp32 tables), case A (helpers_library.law_case, 35 states), beta = (1, 1/2), a swap
behind every iteration, joint start (17, 3), 2^16 ensembles:
  a recorder that read the slot BEFORE the swap would draw rung 0's row after one iteration from the pre-swap law: expected Pearson
    299 701 against a bound of 75.2 at 34 degrees of freedom (from the equal start (17, 17) only 3 335, hence the unequal start);
  rung 0's marginal of the joint law after 64 iterations is within 1.6e-8 of exp(E)/Z in total variation (bound 1e-6);
  reading rung 1 as rung 0 after 64 iterations would score 37 416 against 75.2."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht

N_GPU = 1 << 16          # ensembles of the GPU law test


# ------------------------------------------------------------------------------------------------ the row schedule
def test_row_schedule_at_its_edges():
    from ppde_amd.sampler import recorder_row_of, recorder_rows, recorder_rows_done
    T = 130
    # burn_in = 0, every = 1: every iteration, row t - 1
    assert recorder_rows(T, 0, 1) == T
    assert recorder_row_of(0, 0, 1) is None and recorder_row_of(1, 0, 1) == 0 and recorder_row_of(T, 0, 1) == T - 1
    # burn_in + every = max_steps: exactly one row, filled by the last iteration
    for burn_in, every in ((0, T), (T - 1, 1), (T - 7, 7)):
        assert recorder_rows(T, burn_in, every) == 1
        assert [t for t in range(T + 1) if recorder_row_of(t, burn_in, every) is not None] == [T]
        assert recorder_row_of(T, burn_in, every) == 0
        assert recorder_rows_done(T - 1, burn_in, every) == 0 and recorder_rows_done(T, burn_in, every) == 1
    # one step further and nothing fits
    for burn_in, every in ((0, T + 1), (T, 1), (T - 3, 4), (T + 5, 1)):
        assert recorder_rows(T, burn_in, every) == 0
    # the general rule: t > burn_in and (t - burn_in) % every == 0 -> row (t - burn_in) / every - 1; rows are filled in order,
    # without gaps, and rows_done after t iterations counts exactly the rows filled so far
    for burn_in, every in ((0, 1), (3, 4), (5, 10), (0, 7), (129, 1), (64, 33)):
        filled = [(t, recorder_row_of(t, burn_in, every)) for t in range(T + 1)]
        rows = [r for _, r in filled if r is not None]
        assert rows == list(range(recorder_rows(T, burn_in, every)))
        for t, r in filled:
            if r is not None:
                assert t == burn_in + (r + 1) * every
            assert recorder_rows_done(t, burn_in, every) == sum(1 for t2, r2 in filled if r2 is not None and t2 <= t)
    assert recorder_row_of(3, 3, 4) is None and recorder_row_of(7, 3, 4) == 0 and recorder_row_of(8, 3, 4) is None


# ------------------------------------------------------------------------------------------------ PPDE_PAS
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


def test_ppde_pas_sampling_refusals_come_before_any_device_work():
    from ppde_amd.sampler import PPDE_PAS
    s = PPDE_PAS(_args())
    assert s.sample_every == 0 and s.samples is None                                          # off by default
    ladder = dict(ppde_reversible=True, ppde_betas=(1.0, 0.5, 0.25))
    assert PPDE_PAS(_args(ppde_sample_every=5)).sample_rung is None                           # all chains without a ladder
    assert PPDE_PAS(_args(ppde_sample_every=5, **ladder)).sample_rung == 0                    # the beta[0] sample with one
    assert PPDE_PAS(_args(ppde_sample_every=5, ppde_sample_rung=2, **ladder)).sample_rung == 2
    for bad, what in ((dict(ppde_sample_every=-1), "ppde_sample_every"),
                      (dict(ppde_sample_burn_in=3), "need ppde_sample_every"),
                      (dict(ppde_sample_counts_only=True), "need ppde_sample_every"),
                      (dict(ppde_sample_rung=0), "need ppde_sample_every"),
                      (dict(ppde_sample_every=2, ppde_sample_burn_in=-1), "ppde_sample_burn_in"),
                      (dict(ppde_sample_every=2, ppde_sample_rung=0), "needs a ladder"),
                      (dict(ppde_sample_every=2, ppde_streams=2), "ppde_streams"),
                      (dict(ppde_sample_every=2, ppde_sample_rung=3, **ladder), "rung of the ladder"),
                      (dict(ppde_sample_every=2, ppde_sample_rung=-1, **ladder), "rung of the ladder")):
        with pytest.raises(ValueError, match=what):
            PPDE_PAS(_args(**bad))
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    x0, c = _x0(6)
    for kw in (dict(ppde_sample_every=6), dict(ppde_sample_every=1, ppde_sample_burn_in=5), dict(ppde_sample_every=3, ppde_sample_burn_in=3)):
        with pytest.raises(ValueError, match="no iteration of 5 would be recorded"):
            PPDE_PAS(_args(**kw)).run(x0, 5, ef, 0, c["L"] - 1, None)
    # a schedule that fits goes on to the device (here: to the stand-in, which says so)
    with pytest.raises(AssertionError, match="touched the model"):
        PPDE_PAS(_args(ppde_sample_every=5)).run(x0, 5, ef, 0, c["L"] - 1, None)


def test_cli_flags_parse_into_the_sampler_arguments():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli_rec", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--ppde_sample_every", "10", "--ppde_sample_burn_in", "100", "--ppde_sample_rung", "1",
                                       "--ppde_sample_counts_only"])
    assert (a.ppde_sample_every, a.ppde_sample_burn_in, a.ppde_sample_rung, a.ppde_sample_counts_only) == (10, 100, 1, True)
    d = mod.build_parser().parse_args([])
    assert (d.ppde_sample_every, d.ppde_sample_burn_in, d.ppde_sample_rung, d.ppde_sample_counts_only) == (0, 0, None, False)
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(argparse.Namespace(**{**vars(d), "ppde_library": None})).sample_every == 0   # the defaults switch nothing on


# ------------------------------------------------------------------------------------------------ the host layer
def test_host_layer_of_the_recorder_under_address_sanitizer():
    """tests/hostcheck/recorder.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime of
    tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: every refusal, then a valid recorder, init, run, shape, read
    and destroy, then the walk once per fallible runtime call with that call failing. Any leak or out-of-bounds access fails the
    run."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "recorder", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck recorder ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ the power of the rung test
@pytest.fixture(scope="module")
def case_a():
    c = ht.case_a()
    Ks, states, index, E, inside = ht.kernels_of(c, ht.BETAS_A, 2)
    return c, Ks, states, index, E, inside


def test_the_gpu_law_test_can_see_a_slot_read_before_the_swap(case_a):
    _, Ks, states, _, E, _ = case_a
    S = states.shape[0]
    assert S == 35

    def rung0_after_one(start, swap_every):
        return ht.joint_law(1, Ks, E, ht.BETAS_A, swap_every, start[0] * S + start[1]).reshape(S, S).sum(1)

    stats = {}
    for start in (ht.POWER_START_A, (17, 17)):
        true, before = rung0_after_one(start, 1), rung0_after_one(start, 0)                 # (before the swap: rung 0's own kernel row)
        assert np.abs(before - Ks[0][start[0]]).max() <= 1e-12
        stat, df = ht.expected_pearson(true, before, N_GPU)
        stats[start] = stat
        print(f"slot read before the swap, start {start}: expected Pearson {stat:.0f} on {df} degrees of freedom "
              f"(bound {hl.chi_square_bound(df):.1f})")
        assert df == 34
    bound = hl.chi_square_bound(34)
    assert stats[ht.POWER_START_A] >= 100.0 * bound                                          # far outside: 299 701 against 75.2
    assert stats[ht.POWER_START_A] >= 10.0 * stats[(17, 17)]                                 # hence the unequal start


def test_rung_zero_reaches_exp_energy_over_Z_and_rung_one_does_not(case_a):
    _, Ks, states, _, E, inside = case_a
    S = states.shape[0]
    start = ht.POWER_START_A
    joint = ht.joint_law(64, Ks, E, ht.BETAS_A, 1, start[0] * S + start[1]).reshape(S, S)
    pi = hr.target_law(E, inside)
    tv = hr.total_variation(joint.sum(1), pi)
    print(f"TV(rung 0's marginal after 64 iterations, exp(E)/Z) {tv:.2e}")
    assert tv <= 1e-6
    stat, df = ht.expected_pearson(pi, joint.sum(0), N_GPU)                                  # rung 1 read as rung 0
    print(f"rung 1 read as rung 0 after 64 iterations: expected Pearson {stat:.0f} on {df} degrees of freedom "
          f"(bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10 and stat >= 100.0 * hl.chi_square_bound(df)

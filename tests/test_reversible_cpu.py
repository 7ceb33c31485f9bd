"""Reversible mode without a GPU: the reference of tests/helpers_reversible.py is a Metropolis-Hastings chain for exp(E)/Z
(enumerated kernel, detailed balance, stationary vector), the enumeration agrees with the reference's own sampler, the
shipped accept ratio fails the same yardstick by orders of magnitude, the replay cases of tests/test_reversible_gpu.py keep
their distance from ties, and PPDE_PAS refuses what the mode cannot serve before it touches a device.

Bounds: detailed-balance residual 5e-6 (ten times the fp32 noise of the reference's own probabilities, which enter the
enumeration as products of up to six of them; measured 4.0e-7 / 2.9e-7), total variation 1e-6 (measured 9e-8 / 5e-8), rows
summing to 1 within 1e-6."""
import argparse

import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_reversible as hr
import ppde_oracle as orc

PAS = 2


@pytest.fixture(scope="module")
def law():
    c = dict(hl.law_case(), cnn=None, lamda=0.0)
    en = hl.oracle_energy_of(c)
    K, states, index, e, inside = hr.exact_reversible_kernel(en, c["wt"], c["allowed"], PAS, 0, c["L"] - 1, 0)
    return c, en, K, states, index, e, inside


def _assert_reversible(K, pi):
    rows = np.abs(K.sum(1) - 1.0).max()
    res = hr.detailed_balance_residual(K, pi)
    tv = hr.total_variation(hr.stationary_vector(K), pi)
    print(f"rows sum to 1 within {rows:.2e}; detailed-balance residual {res:.2e}; TV(stationary, exp(E)/Z) {tv:.2e}")
    assert rows <= 1e-6
    assert res <= 5e-6
    assert tv <= 1e-6


def test_enumerated_kernel_is_in_detailed_balance_with_exp_energy(law):
    c, _, K, states, _, e, inside = law
    assert inside.all() and states.shape[0] == 35
    _assert_reversible(K, hr.target_law(e, inside))


def test_enumerated_kernel_under_the_cap_is_in_detailed_balance_on_the_states_inside_it():
    c = hr.cap_case()
    en = hl.oracle_energy_of(c)
    K, states, _, e, inside = hr.exact_reversible_kernel(en, c["wt"], c["allowed"], PAS, 0, c["L"] - 1, c["nmut"])
    assert inside.sum() >= 20 and not inside.all()
    assert np.abs(K[np.ix_(inside, ~inside)]).max() == 0.0                    # no state inside the cap ever leaves it
    _assert_reversible(K[np.ix_(inside, inside)], hr.target_law(e, inside)[inside])


def test_the_shipped_accept_ratio_fails_the_same_yardstick(law):
    """Power of the yardstick: the existing enumeration of the reference's accept ratio on the same model."""
    c, en, _, _, _, e, inside = law
    K0, _, _ = hl.exact_library_kernel(en, c["wt"], c["allowed"], PAS, 0, c["L"] - 1, 0)
    pi = hr.target_law(e, inside)
    res, tv = hr.detailed_balance_residual(K0, pi), hr.total_variation(hr.stationary_vector(K0), pi)
    print(f"reference accept ratio: detailed-balance residual {res:.4f}, TV {tv:.3f}")
    assert res > 0.5 and tv > 0.1


@pytest.mark.parametrize("two_level", [False, True])
def test_enumeration_against_the_reversible_sampler(law, two_level):
    """40 000 chains of reversible_run on torch's noise, one iteration from two start states, flat race and two-level draw."""
    c, en, K, states, index, _, _ = law
    n, L, S = 40000, c["L"], states.shape[0]
    gen = torch.Generator().manual_seed(11)
    for start in (index[(int(c["wt"][2]), int(c["wt"][3]))], 17):
        U, q, u = orc.draw_noise_torch(n, L + 20 if two_level else L * 20, PAS, generator=gen)
        x = states[start].repeat(n, 1)
        ref = hr.reversible_run(en, x, c["wt"], lambda t: (U, q, u), 1, 0, L - 1, PAS, 0, allowed=c["allowed"])
        cells, forbidden = hl.state_cells(ref["final_idx"].numpy(), c["allowed"], index, states[start].numpy())
        assert forbidden == 0
        chi2, df = hl.chi_square(np.bincount(cells, minlength=S).astype(np.float64), n * K[start])
        print(f"start {start} two_level={two_level}: chi2 {chi2:.1f} on {df} degrees of freedom")
        assert df >= 10 and chi2 < hl.chi_square_bound(df), (start, chi2, df)


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("name", sorted(hr.REPLAY_CASES))
def test_replay_cases_keep_their_distance_from_ties(name, rng_mode):
    """On the reference alone: exact equality of draws and accept bits on the GPU is a fair demand only if no decision of the
    run sits on a rounding error."""
    c, lib = hr.replay_model()
    noise, ref = hr.replay_reference(name, rng_mode, hl.oracle_energy_of(c), c, lib, keep_probs=True)
    acc_margin, gap = hr.replay_margins(noise, ref)
    print(f"{name} rng_mode {rng_mode}: smallest |log_acc - log u| {acc_margin:.3g}, smallest race gap {gap:.3g}")
    assert acc_margin > 2e-3
    assert gap > 1e-4
    if hr.REPLAY_CASES[name]["nmut"]:
        capped = torch.stack([(o["proposal"] != torch.as_tensor(c["wt"].astype(np.int64))).sum(-1) >= hr.REPLAY_CASES[name]["nmut"]
                              for o in ref["traces"]])
        assert capped.any() and ref["accepted"].any() and not (capped & ref["accepted"]).any()


class _NoDevice:
    """Stands where the energy function's model would: any use of it is a device call the refusal must come before."""
    which = 1

    def __getattr__(self, name):
        raise AssertionError(f"PPDE_PAS touched the model ({name}) before refusing")


def _args(**kw):
    return argparse.Namespace(ppde_pas_length=2, nmut_threshold=0, paper_results=False, ppde_rng="philox", seed=1, **kw)


def test_ppde_pas_refuses_paper_results():
    from ppde_amd.sampler import PPDE_PAS
    a = _args(ppde_reversible=True)
    a.paper_results = True
    with pytest.raises(ValueError, match="paper_results"):
        PPDE_PAS(a)
    assert PPDE_PAS(_args()).reversible is False                              # off by default


def test_ppde_pas_refuses_a_start_state_outside_the_library():
    from ppde_amd.encoding import idx_to_onehot
    from ppde_amd.sampler import PPDE_PAS
    c = hl.law_case()
    wt = c["wt"].astype(np.int64)
    x0 = np.tile(wt, (4, 1))
    outside = next(k for k in range(20) if not (int(c["allowed"][2]) >> k) & 1)
    x0[3, 2] = outside
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    s = PPDE_PAS(_args(ppde_reversible=True, ppde_library=c["allowed"]))
    with pytest.raises(ValueError, match=r"chain 3 .* open residue 2"):
        s.run(torch.from_numpy(idx_to_onehot(x0.astype(np.uint8))).float(), 5, ef, 0, c["L"] - 1, None)
    # without a library the mode opens [min_pos, max_pos] with every letter: any population passes the check and the run goes on
    # to the device (here: to the stand-in, which says so)
    with pytest.raises(AssertionError, match="touched the model"):
        PPDE_PAS(_args(ppde_reversible=True)).run(torch.from_numpy(idx_to_onehot(x0.astype(np.uint8))).float(), 5, ef, 2, 3, None)


def test_host_layer_of_reversible_mode_under_address_sanitizer():
    """tests/hostcheck/reversible.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime
    of tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: create -> set_library -> set_reversible -> init -> run
    -> collect -> destroy on both RNG modes and gradient policies, the refusals, then the walk once per fallible runtime call
    with that call failing. Any leak or out-of-bounds access fails the run."""
    import os
    import re
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "reversible", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck reversible ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

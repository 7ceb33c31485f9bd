"""Parallel tempering without a GPU: the reference of tests/helpers_tempering.py keeps the product law
prod_r exp(beta_r E(x_r)) / Z_r (enumerated joint kernel), `tempered_run` agrees with that enumeration, the GPU law test of
tests/test_tempering_gpu.py has the power to see a wrong swap rule, its replay cases keep their distance from ties, and
PPDE_PAS refuses what the mode cannot serve before it touches a device.

Bounds are tests/test_reversible_cpu.py's: detailed-balance residual 5e-6, total variation 1e-6, rows summing to 1 within 1e-6.

Enumerated (CPU, fp64 over the reference's fp32 tables):
  case A (helpers_library.law_case, 35 states, beta = (1, 1/2), pas_length 2): each K_beta in detailed balance with
    exp(beta E)/Z (residual 4.0e-7 / 2.9e-7, TV 1.7e-8 / 1.9e-8); stationary vector of the joint kernel against the product
    law TV 2.5e-8; K^64 row against it 2.4e-8.
  case B (one residue, 5 letters, beta = (1, 1/2, 1/4, 1/8), swap_every 2): joint law after 32 iterations against the product
    law TV 2.4e-8.
  power: on case A the joint law after T = 1 differs from the law without the swap by 0.093 in total variation, after T = 12 by
    1.5e-4 only: the T = 1 and T = 2 rows of the GPU law test carry the swap check.
  a finding of the power test: from the wild type on both rungs (equal energies, d = 0 in the first event) a swap rule formed
    from beta-scaled energies is barely visible at T = 1 (expected Pearson 1488 on 772 degrees of freedom, bound 968) and ignored
    parity at T = 2 not at all (1132 on 900, bound 1112). From the joint start state (17, 3) -- different states on the two
    rungs -- all three planted faults exceed twice the bound (sign 234024 and scaled 12159 on 795 at T = 1, parity 8874 on 860
    at T = 2), so the GPU law test's second T = 1 row and its T = 2 rows start there (helpers_tempering.POWER_START_A)."""
import argparse

import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht
import ppde_oracle as orc

PAS = 2
N_GPU_A = 1 << 16          # ensembles of the GPU law test on case A


@pytest.fixture(scope="module")
def case_a():
    c = ht.case_a()
    Ks, states, index, E, inside = ht.kernels_of(c, ht.BETAS_A, PAS)
    return c, Ks, states, index, E, inside


@pytest.fixture(scope="module")
def case_b():
    c = ht.case_b()
    Ks, states, index, E, inside = ht.kernels_of(c, ht.BETAS_B, PAS)
    return c, Ks, states, index, E, inside


def test_each_rung_is_in_detailed_balance_with_its_own_law(case_a):
    _, Ks, states, _, E, inside = case_a
    assert states.shape[0] == 35 and inside.all()
    for b, K in zip(ht.BETAS_A, Ks):
        pi = hr.target_law(b * E, inside)
        res, tv = hr.detailed_balance_residual(K, pi), hr.total_variation(hr.stationary_vector(K), pi)
        print(f"beta {b}: rows {np.abs(K.sum(1) - 1).max():.2e}, detailed-balance residual {res:.2e}, TV {tv:.2e}")
        assert np.abs(K.sum(1) - 1.0).max() <= 1e-6 and res <= 5e-6 and tv <= 1e-6


def test_joint_kernel_keeps_the_product_law(case_a):
    _, Ks, _, _, E, _ = case_a
    K = ht.exact_tempered_kernel(Ks, E, ht.BETAS_A, 0)
    assert K.shape == (1225, 1225) and np.abs(K.sum(1) - 1.0).max() <= 1e-6
    tv = hr.total_variation(hr.stationary_vector(K), ht.product_law(E, ht.BETAS_A))
    print(f"case A: TV(stationary of the joint kernel, product law) {tv:.2e}")
    assert tv <= 1e-6
    # parity 1 has no pair with two rungs: the swap matrix is the identity
    assert np.array_equal(ht.swap_matrix(E, ht.BETAS_A, 1), np.eye(1225))


def test_four_rungs_reach_the_product_law(case_b):
    _, Ks, states, _, E, _ = case_b
    assert states.shape[0] == 5
    v = ht.joint_law(32, Ks, E, ht.BETAS_B, ht.SWAP_EVERY_B, 0)
    tv = hr.total_variation(v, ht.product_law(E, ht.BETAS_B))
    print(f"case B: TV(joint law after 32 iterations, product law) {tv:.2e}")
    assert v.shape == (625,) and abs(v.sum() - 1.0) <= 1e-6 and tv <= 1e-6


def test_equilibrium_row_of_case_a(case_a):
    c, Ks, _, index, E, _ = case_a
    start = index[(int(c["wt"][2]), int(c["wt"][3]))]
    v = ht.joint_law(64, Ks, E, ht.BETAS_A, 1, start * 35 + start)
    tv = hr.total_variation(v, ht.product_law(E, ht.BETAS_A))
    print(f"case A: TV(K^64 row, product law) {tv:.2e}")
    assert tv <= 1e-6


def test_the_gpu_law_test_can_see_the_swap(case_a):
    """The T = 1 row carries the swap check (T = 12 has forgotten it), and each of three planted faults of the swap rule would
    push the GPU law test's Pearson statistic, at its sample size, to at least twice its bound."""
    c, Ks, _, index, E, _ = case_a
    start = index[(int(c["wt"][2]), int(c["wt"][3]))]
    j0 = start * 35 + start
    with_swap = {T: ht.joint_law(T, Ks, E, ht.BETAS_A, 1, j0) for T in (1, 12)}
    without = {T: ht.joint_law(T, Ks, E, ht.BETAS_A, 0, j0) for T in (1, 12)}
    j1 = ht.POWER_START_A[0] * 35 + ht.POWER_START_A[1]
    with_swap_1 = {T: ht.joint_law(T, Ks, E, ht.BETAS_A, 1, j1) for T in (1, 2)}
    tv1, tv12 = hr.total_variation(with_swap[1], without[1]), hr.total_variation(with_swap[12], without[12])
    print(f"TV(with swap, without) at T=1 {tv1:.3f}, at T=12 {tv12:.2e}")
    assert tv1 > 0.05 and tv12 < 1e-3
    for fault in ("sign", "scaled", "parity"):
        # 'parity' only shows where an odd event takes place: the second iteration
        T = 2 if fault == "parity" else 1
        stat, df = ht.expected_pearson(with_swap_1[T], ht.joint_law(T, Ks, E, ht.BETAS_A, 1, j1, fault=fault), N_GPU_A)
        print(f"fault {fault!r} at T={T}: expected Pearson {stat:.0f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.0f})")
        assert df >= 10 and stat >= 2.0 * hl.chi_square_bound(df), (fault, stat, df)


@pytest.mark.parametrize("two_level", [False, True])
def test_enumeration_against_the_tempered_sampler(case_a, two_level):
    """40 000 ensembles of tempered_run on torch's noise (swap uniforms included), two iterations from two joint start states:
    the statistic and bound of test_enumeration_against_the_reversible_sampler."""
    c, Ks, states, index, E, _ = case_a
    R, S, L, n_ens = 2, 35, c["L"], 40000
    n = n_ens * R
    en = hl.oracle_energy_of(c)
    gen = torch.Generator().manual_seed(13)
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    for s0, s1 in ((wt_row, wt_row), ht.POWER_START_A):
        T = 2
        noise = [orc.draw_noise_torch(n, L + 20 if two_level else L * 20, PAS, generator=gen) for _ in range(T)]
        su = [torch.rand(n_ens, R, generator=gen).numpy() for _ in range(T)]
        x = torch.stack([states[s0], states[s1]]).repeat(n_ens, 1)
        ref = ht.tempered_run(en, x, c["wt"], lambda t: noise[t], T, 0, L - 1, PAS, 0, ht.BETAS_A, 1, allowed=c["allowed"],
                              swap_u=lambda t: su[t])
        assert ref["swap_attempts"].sum() == n_ens and 0 < ref["swap_accepts"].sum() < n_ens      # one even event in two iterations
        cells0, bad0 = hl.state_cells(ref["final_idx"].numpy()[0::2], c["allowed"], index, states[s0].numpy())
        cells1, bad1 = hl.state_cells(ref["final_idx"].numpy()[1::2], c["allowed"], index, states[s1].numpy())
        assert bad0 == 0 and bad1 == 0
        both = np.stack([cells0, cells1], 1)
        by_rung = np.take_along_axis(both, np.argsort(ref["rung"].reshape(n_ens, R), 1), 1)
        joint = by_rung[:, 0] * S + by_rung[:, 1]
        expected = ht.joint_law(T, Ks, E, ht.BETAS_A, 1, s0 * S + s1)
        chi2, df = hl.chi_square(np.bincount(joint, minlength=S * S).astype(np.float64), n_ens * expected)
        print(f"start ({s0}, {s1}) two_level={two_level}: chi2 {chi2:.1f} on {df} degrees of freedom")
        assert df >= 10 and chi2 < hl.chi_square_bound(df), (chi2, df)


@pytest.mark.parametrize("name,rng_mode,swap_every",
                         [(nm, 0, 0) for nm in sorted(ht.REPLAY_CASES)] +
                         [(nm, 1, sw) for nm in sorted(ht.REPLAY_CASES) for sw in ht.REPLAY_SWAPS])
def test_tempering_replay_cases_keep_their_distance_from_ties(name, rng_mode, swap_every):
    """On the reference alone (test_replay_cases_keep_their_distance_from_ties' margins, and the same for |d - log u| of the
    swap decisions): exact equality on the GPU is a fair demand only if no decision sits on a rounding error. The device-RNG
    runs with an exchange are checked over the longer of the GPU test's two lengths."""
    c, lib = hr.replay_model()
    T = ht.T_DEV_LONG if rng_mode == 1 and swap_every else None
    noise, ref = ht.replay_reference(name, rng_mode, swap_every, hl.oracle_energy_of(c), c, lib, keep_probs=True, T=T)
    acc_margin, gap = hr.replay_margins(noise, ref)
    print(f"{name} rng_mode {rng_mode} swap_every {swap_every}: smallest |log_acc - log u| {acc_margin:.3g}, race gap {gap:.3g}, "
          f"swap margin {ref['swap_margin']:.3g}; swaps {ref['swap_accepts'].sum()} / {ref['swap_attempts'].sum()}")
    assert acc_margin > 2e-3
    assert gap > 1e-4
    assert ref["swap_margin"] > 2e-3
    first = ref["accepted"][:20]                                             # (the shorter GPU run sees acceptances and rejections too)
    assert first.any() and not first.all()
    if swap_every:
        assert 0 < ref["swap_accepts"].sum() < ref["swap_attempts"].sum()
        assert (ref["rung_history"][-1] != ref["rung_history"][0]).any()


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


def test_ppde_pas_tempering_refusals_come_before_any_device_work():
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(_args()).betas is None and PPDE_PAS(_args()).swap_every == 1                 # off by default
    with pytest.raises(ValueError, match="ppde_reversible"):
        PPDE_PAS(_args(ppde_betas=(1.0, 0.5)))
    for bad, what in (((1.0, 1.0), "strictly decreasing"), ((0.5, 1.0), "strictly decreasing"), ((1.0, 0.0), "positive"),
                      ((1.0, float("nan")), "finite"), ((1.0, -0.5), "positive"), ((float("inf"), 1.0), "finite"),
                      (tuple(2.0 ** -i for i in range(65)), "64")):
        with pytest.raises(ValueError, match=what):
            PPDE_PAS(_args(ppde_reversible=True, ppde_betas=bad))
    with pytest.raises(ValueError, match="ppde_swap_every"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_betas=(1.0, 0.5), ppde_swap_every=-1))
    with pytest.raises(ValueError, match="ppde_streams"):
        PPDE_PAS(_args(ppde_reversible=True, ppde_betas=(1.0, 0.5), ppde_streams=2))
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    x0, c = _x0(6)
    s = PPDE_PAS(_args(ppde_reversible=True, ppde_betas=(1.0, 0.5, 0.25, 0.125), ppde_library=c["allowed"]))
    with pytest.raises(ValueError, match="multiple of the 4 rungs"):
        s.run(x0, 5, ef, 0, c["L"] - 1, None)
    # a population that fits goes on to the device (here: to the stand-in, which says so)
    x0, c = _x0(8)
    with pytest.raises(AssertionError, match="touched the model"):
        s.run(x0, 5, ef, 0, c["L"] - 1, None)


def test_ppde_pas_refuses_a_shard_boundary_inside_an_ensemble(monkeypatch):
    from ppde_amd import sampler
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    x0, c = _x0(12)
    s = sampler.PPDE_PAS(_args(ppde_reversible=True, ppde_betas=(1.0, 0.5, 0.25, 0.125), ppde_library=c["allowed"], ppde_shard=True))
    monkeypatch.setattr(sampler, "world", lambda: (1, 2))                                        # 12 chains over 2 ranks: 6 + 6
    with pytest.raises(ValueError, match="shard boundary"):
        s.run(x0, 5, ef, 0, c["L"] - 1, None)


def test_cli_flags_parse_into_the_sampler_arguments():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--ppde_betas", "1,0.7,0.5,0.35", "--ppde_swap_every", "5", "--ppde_reversible"])
    assert a.ppde_betas == [1.0, 0.7, 0.5, 0.35] and a.ppde_swap_every == 5
    d = mod.build_parser().parse_args([])
    assert d.ppde_betas is None and d.ppde_swap_every == 1


def test_host_layer_of_tempering_under_address_sanitizer():
    """tests/hostcheck/tempering.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime
    of tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: create -> set_library -> set_reversible ->
    set_tempering (every refusal, then a valid ladder) -> init -> run -> tempering_state / history -> destroy, then the walk once
    per fallible runtime call with that call failing. Any leak or out-of-bounds access fails the run."""
    import os
    import re
    import subprocess
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "tempering", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck tempering ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

"""The expert-set x mode matrix without a GPU (tests/helpers_modes.py): the `DeviceEnergy` adaptor is transparent, the comparison
tests/test_modes_gpu.py runs has the power to see the faults of the chain-kernel glue that no Potts / CNN run can show, and its
replay configurations keep their distance from ties.

The stand-in under the adaptor is `helpers_modes.OracleModel`: the CPU oracle (Potts, CNN ensemble, the ESM-2 restatement with the
device's fp16 rounding points) of the GPU module's toy model, served through the HIP model's `energy_grad(idx, which)`.

Planted faults, each on the reference side of `compare_replay` against the fault-free run in the device's layout, at the GPU
replays' own T = 20 and n = 16 and on the noise the device RNG draws for them:
  the transformer term missing from the accept ratio's energy; lamda * d fit / dx in the proposal rows without bit 3, and missing
  with it; e_x read from the proposal's slot; beta on the rows but not on e_y - e_x; for which = 2 the swap decided on fit * lamda.
Each must be rejected by a draw, an accept bit, log_acc or the rung history -- a real difference, never a validated near-tie."""
import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_modes as hm
import helpers_reversible as hr
import helpers_tempering as ht
import ppde_oracle as orc

LAW_N = 1 << 16                      # chains of the GPU law tests


@pytest.fixture(scope="module")
def toy():
    model, wt = hm.oracle_model()
    return model, wt, hm.window_library(wt, hm.TOY["win"])


def _noise(which, mode, rng_mode, L):
    if rng_mode == 0:
        return hm.torch_noise(which, mode, hm.N, L)
    return [orc.device_noise(hm.philox_seed(which, mode), 0, hm.N, t, hm.PAS, L) for t in range(hm.T)]


_RUNS = {}


def _good(toy, which, mode, rng_mode=1):
    key = (which, mode, rng_mode)
    if key not in _RUNS:
        model, wt, lib = toy
        noise = _noise(which, mode, rng_mode, len(wt))
        ref = hm.reference_run(mode, hm.DeviceEnergy(model, which), wt, lib, noise, hm.TOY["win"], hm.philox_seed(which, mode))
        _RUNS[key] = (noise, ref)
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. the adaptor is transparent
@pytest.mark.parametrize("which,mode", [(7, "default_lib"), (6, "rev_lib"), (7 | 8, "temp_sw1"), (2, "temp_lib"), (5, "rev")])
def test_a_run_through_the_adaptor_is_the_run_on_the_oracle(toy, which, mode):
    model, wt, lib = toy
    noise, ref = _good(toy, which, mode)
    if which == 2:
        class Supervised:                                                     # e = fit, g = d fit / dx: ProteinSupervised
            energy = staticmethod(lambda idx: (model.cnn.fit_grad(idx, want_grad=False)[0],) * 2)
            energy_grad = staticmethod(lambda idx: (lambda f, g: (f, f, g))(*model.cnn.fit_grad(idx)))
        direct = Supervised
    else:
        direct = orc.EnergyOracle(model.potts if which & 1 else None, model.cnn if which & 2 else None, model.lamda, tf=model.tf,
                                  full_grad=bool(which & 8))
    ref2 = hm.reference_run(mode, direct, wt, lib, noise, hm.TOY["win"], hm.philox_seed(which, mode))
    for k in ("energy_history", "fitness_history", "best_idx", "states", "accepted", "final_idx"):
        assert torch.equal(ref[k], ref2[k]), k
    for a, b in zip(ref["traces"], ref2["traces"]):
        assert torch.equal(a["flat"], b["flat"]) and torch.equal(a["log_acc"], b["log_acc"]) and torch.equal(a["p_fwd"], b["p_fwd"])
    if "rung_history" in ref:
        for k in ("rung_history", "rung", "beta", "swap_attempts", "swap_accepts"):
            assert np.array_equal(ref[k], ref2[k]), k
    # ... and a fault-free run in the device's layout passes the GPU module's comparison against itself, bit-equal
    out = hm.compare_replay(f"{which}:{mode}", hm.as_device_run(ref, noise, 2 * hm.PAS - 1), ref2, noise,
                            R=len(hm.BETAS) if mode.startswith("temp") else 1, lib=hm.mode_settings(mode, lib)[0])
    assert out["parted"] == [] and out["bit_equal"] and out["log_acc"] == 0.0


def test_the_adaptor_hands_the_device_uint8_states_and_returns_cpu_tensors():
    class Spy:
        def energy_grad(self, idx, which, want_grad=True):
            assert idx.dtype == torch.uint8 and idx.is_contiguous() and which == 6
            n, L = idx.shape
            return torch.arange(n).float(), torch.ones(n), (torch.zeros(n, L, 20) if want_grad else None)

    en = hm.DeviceEnergy(Spy(), 6)
    idx = torch.zeros(3, 24, dtype=torch.int64)
    e, f = en.energy(idx)
    e2, f2, g = en.energy_grad(idx)
    assert e.shape == (3,) and f.shape == (3,) and g.shape == (3, 24, 20) and torch.equal(e, e2) and g.device.type == "cpu"


# ------------------------------------------------------------------------------------------------ 2. the replays' power
def _rejected(tag, good, bad, noise, R, lib):
    with pytest.raises(AssertionError) as info:
        hm.compare_replay(tag, good, bad, noise, R=R, lib=lib)
    msg = str(info.value)
    print(f"[modes power] {tag}: {msg[:160]}")
    # by a decision or the ratio itself; a history alone would not tell this fault from a recording error
    assert any(w in msg for w in ("drew", "accept bit", "log_acc", "rung", "swap")), msg
    return msg


@pytest.mark.parametrize("which,mode,kind", [(7, "rev", "no_tf_in_accept"), (7, "default_lib", "no_tf_in_accept"),
                                             (6, "rev_lib", "no_tf_in_accept"), (5, "temp_sw1", "no_tf_in_accept"),
                                             (7, "rev_lib", "fit_grad_flipped"), (7, "default_lib", "fit_grad_flipped"),
                                             (7 | 8, "rev", "fit_grad_flipped"), (7 | 8, "temp_lib", "fit_grad_flipped"),
                                             (6, "temp_sw2", "fit_grad_flipped"),
                                             (7, "rev", "e_x_from_proposal"), (7, "default_lib", "e_x_from_proposal"),
                                             (7 | 8, "rev_lib", "e_x_from_proposal")])
def test_a_fault_of_the_energy_glue_is_rejected(toy, which, mode, kind):
    model, wt, lib = toy
    noise, ref = _good(toy, which, mode)
    R = len(hm.BETAS) if mode.startswith("temp") else 1
    bad = hm.reference_run(mode, hm.FaultyEnergy(model, which, kind), wt, lib, noise, hm.TOY["win"], hm.philox_seed(which, mode))
    _rejected(f"{which}:{mode}:{kind}", hm.as_device_run(ref, noise, 2 * hm.PAS - 1), bad, noise, R, hm.mode_settings(mode, lib)[0])


@pytest.mark.parametrize("which,mode", [(7, "temp_sw1"), (7, "temp_lib"), (2, "temp_sw2"), (7 | 8, "temp_sw2")])
def test_beta_on_the_rows_alone_is_rejected(toy, which, mode):
    model, wt, lib = toy
    noise, ref = _good(toy, which, mode)
    with hm.beta_on_rows_only():
        bad = hm.reference_run(mode, hm.DeviceEnergy(model, which), wt, lib, noise, hm.TOY["win"], hm.philox_seed(which, mode))
    _rejected(f"{which}:{mode}:beta_on_rows_only", hm.as_device_run(ref, noise, 2 * hm.PAS - 1), bad, noise, len(hm.BETAS),
              hm.mode_settings(mode, lib)[0])


@pytest.mark.parametrize("mode", sorted(m for w, m in hm.PHILOX_SEEDS if w == 2))
def test_a_swap_on_fit_times_lamda_is_rejected_for_the_supervised_expert(toy, mode):
    """The seeded CNNs' fitness spans 0.03 over the states a run visits, so |d| of a swap is ~0.01 and the fault moves about one
    decision in 200: it shows in the cell whose Philox key was picked for it (one in ~100 keys does; none was found for swap_every 2
    or the library cell among 1500). The law test on the scaled CNNs carries this check otherwise (last test of this module)."""
    model, wt, lib = toy
    noise, ref = _good(toy, 2, mode)
    with hm.swap_on_scaled_energy(model.lamda):
        bad = hm.reference_run(mode, hm.DeviceEnergy(model, 2), wt, lib, noise, hm.TOY["win"], hm.philox_seed(2, mode))
    assert not np.array_equal(bad["rung_history"], ref["rung_history"])
    _rejected(f"2:{mode}:swap_on_lamda_fit", hm.as_device_run(ref, noise, 2 * hm.PAS - 1), bad, noise, len(hm.BETAS),
              hm.mode_settings(mode, lib)[0])


# ------------------------------------------------------------------------------------------------ 3. distance from ties
@pytest.mark.parametrize("which,rng_mode", [(w, 1) for w in hm.WHICH] + [(2, 0), (7, 0)])      # torch's noise: expert sets 2 and 7
def test_margins_of_the_replay_configurations(toy, which, rng_mode):
    """Printed, not asserted: the GPU module validates a parting where it happens (its energies are the device's, these the CPU
    oracle's); here one sees how far the reference's decisions of every configuration sit from a tie, and that every
    configuration accepts and rejects."""
    for mode in hm.MODES:
        noise, ref = _good(toy, which, mode, rng_mode)
        acc_margin, gap = hm.margins(noise, ref)
        extra = f", swap margin {ref['swap_margin']:.3g}, swaps {ref['swap_accepts'].sum()} / {ref['swap_attempts'].sum()}" if "swap_margin" in ref else ""
        print(f"which {which} {mode} rng_mode {rng_mode}: smallest |log_acc - log u| {acc_margin:.3g}, race gap {gap:.3g}, "
              f"accepted {float(ref['accepted'].float().mean()):.2f}{extra}")
        assert ref["accepted"].any() and not ref["accepted"].all(), (which, mode)
        if mode.startswith("temp"):
            # (the seeded CNNs' fitness spans 0.03: a which = 2 ladder refuses a swap where its Philox key was picked for it)
            picked = which != 2 or (rng_mode == 1 and (which, mode) in hm.PHILOX_SEEDS)
            assert 0 < ref["swap_accepts"].sum() < ref["swap_attempts"].sum() + (0 if picked else 1), (which, mode)


# ------------------------------------------------------------------------------------------------ 4. the law tests' power
def test_the_law_tests_can_see_a_planted_fault(toy):
    """The GPU law cases at their sample size: the expected Pearson statistic of a planted fault against the enumerated law is
    at least four times the five-sigma bound. which = 7, reversible, one open residue: the transformer term missing from the
    accept energy. which = 2 with the ladder (1, 1/2): the swap decided on fit * lamda."""
    model, wt, _ = toy
    L = len(wt)
    site = hm.LAW_SITE
    allowed = hm.one_site_library(wt, site)
    K, states, index, _, _ = hr.exact_reversible_kernel(hm.DeviceEnergy(model, 7), wt, allowed, hm.PAS, 0, L - 1, 0)
    Kf, *_ = hr.exact_reversible_kernel(hm.FaultyEnergy(model, 7, "no_tf_in_accept"), wt, allowed, hm.PAS, 0, L - 1, 0)
    start = index[(int(wt[site]),)]
    assert np.abs(K.sum(1) - 1.0).max() <= 1e-6
    for T_ in (1, 2, 12):
        stat, df = ht.expected_pearson(hm.population_law(K, start, T_), hm.population_law(Kf, start, T_), LAW_N)
        print(f"which 7 reversible, T={T_}: expected Pearson of the fault {stat:.0f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.0f})")
        assert df >= 10 and stat >= 4.0 * hl.chi_square_bound(df), (T_, stat, df)
    scaled, _ = hm.oracle_model(cnn_gain=hm.LAW_GAIN_2)
    case = dict(wt=wt, allowed=hm.one_site_library(wt, site, hm.LAW_LETTERS_2), L=L, nmut=0)
    Ks, states, index, E, _ = hm.kernels_of(hm.DeviceEnergy(scaled, 2), case, ht.BETAS_A, hm.PAS)
    S = states.shape[0]
    start = hm.law_start_2(E)
    j0 = start[0] * S + start[1]
    print(f"which 2 ladder case: fitness of the {S} states spans {E.max() - E.min():.3f}, start {start}")
    for T_ in (1, 2, 12):
        good = ht.joint_law(T_, Ks, E, ht.BETAS_A, 1, j0)
        # (swap_matrix reads E for the rule alone: the kernels of the rungs are the fault-free ones)
        bad = ht.joint_law(T_, Ks, np.float32(model.lamda) * E.astype(np.float32), ht.BETAS_A, 1, j0)
        stat, df = ht.expected_pearson(good, bad, LAW_N // 2)
        print(f"which 2 ladder {ht.BETAS_A}, T={T_}: expected Pearson of the fault {stat:.0f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.0f})")
        assert df >= 10
        if T_ == 1:                                                          # the row that carries the swap check (test_tempering_cpu.py)
            assert stat >= 4.0 * hl.chi_square_bound(df), (T_, stat, df)

"""Parallel tempering on the GPU (ppde_chains_set_tempering; k_propose_temp, k_accept_temp, k_swap): a ladder of one rung at
beta = 1 is the reversible run bit for bit, a power-of-two ladder replays the reference of tests/helpers_tempering.py exactly
(flat race on torch's noise, two-level draw on the device RNG's own, with and without replica exchange, eager and from graphs),
the joint law of an ensemble follows the enumerated joint kernel and reaches the product law, sharding changes nothing, and the
interfaces around it.

Tolerances are tests/test_reversible_gpu.py's: draws, accept bits, best states, trajectories, rung histories and swap counters
exact (tests/test_tempering_cpu.py shows that no decision of these runs sits near a tie); log acceptance ratios 2e-4, energy
histories 2e-5, fitness 5e-6. The law tests use tests/test_sampler_law.py's statistic and bound; joint cells are (state on rung 0,
state on rung 1, ...), read through tempering_state()["rung"]. The T = 1 and T = 2 rows carry the swap check (the CPU power test
says why, and why the second start state is the one it is)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht
from helpers import device_noise
from ppde_amd import library as dl
from ppde_amd import synthetic
from test_hip_parity import observed

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, betas=None, swap_every=1, x0=None, lo=None, hi=None, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", 99)
    lo = 0 if lo is None else lo
    hi = case["L"] - 1 if hi is None else hi
    ch = Chains(m, n, T, pas, nmut, False, lo, hi, 3 if case.get("cnn") is not None else 1, rng_mode, **kw)
    if lib is not None:
        ch.set_library(lib)
    ch.set_reversible(True)
    if betas is not None:
        ch.set_tempering(betas, swap_every)
    x0 = np.tile(case["wt"], (n, 1)) if x0 is None else x0
    ch.init(torch.as_tensor(x0).cuda())
    return ch


def _feed(ch, noise):
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _assert_same(a, b, tr_a=None, tr_b=None, label=""):
    for k in RESULT_KEYS:
        assert np.array_equal(a[k], b[k]), (label, k)
    if tr_a is not None:
        for k in ("flat", "accepted", "log_acc", "U"):
            assert np.array_equal(tr_a[k], tr_b[k]), (label, k)


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    return c, lib, hl.oracle_energy_of(c)


# ------------------------------------------------------------------------------------------------ 1. beta = 1 is today's run
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_one_rung_at_beta_one_is_the_reversible_run(toy, rng_mode):
    """TOY24, 16 chains, ladder (1.0,), swap_every 0 and 1, both gradient policies, T = 20: every result and trace array equals
    the reversible run without tempering bit for bit (whose reuse run on the device RNG goes through the fused kernel)."""
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    n, T, lo, hi = 16, 20, c["i0"], c["i0"] + c["Lp"] - 1
    gen = torch.Generator().manual_seed(77)
    import ppde_oracle as orc
    noise = [orc.draw_noise_torch(n, c["L"] * 20, 2, generator=gen) for _ in range(T)] if rng_mode == 0 else None
    for reuse in (True, False):
        out = []
        for betas, sw in ((None, 0), ((1.0,), 0), ((1.0,), 1)):
            ch = _chains(m, c, n, T, 2, 3, rng_mode, lib, betas, sw, lo=lo, hi=hi, trace=True, reuse_grad=reuse)
            if rng_mode == 0:
                _feed(ch, noise)
            else:
                ch.run(T)
            out.append((ch.collect(), ch.trace()))
            if betas is not None:
                st = ch.tempering_state()
                assert (st["rung"] == 0).all() and (st["beta"] == 1.0).all() and st["swap_attempts"].shape == (n, 0)
                assert (ch.tempering_history() == 0).all()
            ch.close()
        assert out[0][1]["accepted"].any() and not out[0][1]["accepted"].all()
        for k in (1, 2):
            _assert_same(out[0][0], out[k][0], out[0][1], out[k][1], label=f"rng_mode={rng_mode} reuse={reuse} variant={k}")
    m.close()


# ------------------------------------------------------------------------------------------------ 2.-3. replays
def _assert_against_reference(tag, tr, res, ref, noise, T, lib, check_U=False):
    ok = dl.as_bool(lib).reshape(-1)
    for t in range(T):
        U = noise[t][0].numpy()
        if check_U:
            assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
            assert ok[tr["flat"][t, s][act]].all()
    ref_la = np.stack([o["log_acc"].numpy() for o in ref["traces"]])
    la = observed(f"tempering:{tag}:log_acc", np.abs(tr["log_acc"] - ref_la), 2e-4)
    en = observed(f"tempering:{tag}:energy", np.abs(res["energy_history"] - ref["energy_history"].numpy()), 2e-5)
    fi = observed(f"tempering:{tag}:fitness", np.abs(res["fitness_history"] - ref["fitness_history"].numpy()), 5e-6)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy())
    assert la <= 1.0 and en <= 1.0 and fi <= 1.0


def _assert_tempering_state(ch, ref, label):
    st, hist = ch.tempering_state(), ch.tempering_history()
    assert np.array_equal(hist, ref["rung_history"]), label
    assert np.array_equal(st["rung"], ref["rung"]) and np.array_equal(st["beta"], ref["beta"]), label
    assert np.array_equal(st["swap_attempts"], ref["swap_attempts"]) and np.array_equal(st["swap_accepts"], ref["swap_accepts"]), label


def _replay_chains(m, c, lib, k, rng_mode, swap_every, T=None, **kw):
    return _chains(m, c, k["n"], k["T"] if T is None else T, k["pas"], k["nmut"], rng_mode, lib, ht.REPLAY_BETAS, swap_every,
                   lo=c["i0"], hi=c["i0"] + c["Lp"] - 1, seed=k["philox_seed"], **kw)


@pytest.mark.parametrize("name", sorted(ht.REPLAY_CASES))
def test_power_of_two_ladder_replays_the_flat_race(toy, name):
    """rng_mode 0 on torch's noise, ladder (1, 1/2, 1/4, 1/8) without exchange, both gradient policies."""
    c, lib, en = toy
    k = ht.REPLAY_CASES[name]
    noise, ref = ht.replay_reference(name, 0, 0, en, c, lib)
    m = hl.hip_model_of(c)
    out = []
    for reuse in (True, False):
        ch = _replay_chains(m, c, lib, k, 0, 0, trace=True, reuse_grad=reuse)
        _feed(ch, noise)
        tr, res = ch.trace(), ch.collect()
        _assert_against_reference(f"{name}:flat:reuse{int(reuse)}", tr, res, ref, noise, k["T"], lib)
        _assert_tempering_state(ch, ref, name)
        out.append((res, tr))
        ch.close()
    _assert_same(out[0][0], out[1][0], out[0][1], out[1][1])
    assert out[0][1]["accepted"].any()
    m.close()


@pytest.mark.parametrize("swap_every", ht.REPLAY_SWAPS)
@pytest.mark.parametrize("name", sorted(ht.REPLAY_CASES))
def test_power_of_two_ladder_replays_the_device_rng(toy, name, swap_every):
    """rng_mode 1: the reference fed the device's own noise and the swap uniforms restated from Philox; the rung history, the
    final rungs and temperatures and both counters exact; then untraced runs of both gradient policies, eager and replayed from
    hipGraphs (T = 20, and 40 = two replays of the 20-segment), give the same bits."""
    c, lib, en = toy
    k = ht.REPLAY_CASES[name]
    T = k["T_dev"]
    m = hl.hip_model_of(c)
    ch = _replay_chains(m, c, lib, k, 1, swap_every, T=T, trace=True, reuse_grad=False, use_graph=False)
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, k["pas"])
    for t, (U, q, u) in enumerate(ht.replay_noise(name, 1, c["L"])):                         # the noise the CPU margins were checked on
        assert np.array_equal(U.numpy(), noise[t][0].numpy()) and np.array_equal(u.numpy(), noise[t][2].numpy())
    _, ref = ht.replay_reference(name, 1, swap_every, en, c, lib, noise=noise)
    _assert_against_reference(f"{name}:device:swap{swap_every}", tr, res, ref, noise, T, lib, check_U=True)
    _assert_tempering_state(ch, ref, name)
    assert tr["accepted"].any() and not tr["accepted"].all()
    if swap_every:
        assert 0 < ref["swap_accepts"].sum() < ref["swap_attempts"].sum()
    hist = ch.tempering_history()
    for reuse in (False, True):
        for graph in (False, True):
            ch3 = _replay_chains(m, c, lib, k, 1, swap_every, T=T, trace=False, reuse_grad=reuse, use_graph=graph)
            ch3.run(T)
            assert ch3.graph_stats()["replayed_steps"] == (T if graph else 0)
            _assert_same(res, ch3.collect(), label=f"reuse={reuse} graph={graph}")
            assert np.array_equal(ch3.tempering_history(), hist)
            ch3.close()
    ch.close()
    if swap_every:
        # the longer run: two replays of the 20-iteration segment against the reference over 40 iterations
        T2 = ht.T_DEV_LONG
        noise2, ref2 = ht.replay_reference(name, 1, swap_every, en, c, lib, T=T2)
        ch4 = _replay_chains(m, c, lib, k, 1, swap_every, T=T2, trace=True, reuse_grad=True, use_graph=True)
        ch4.run(T2)
        assert ch4.graph_stats()["replayed_steps"] == T2
        _assert_against_reference(f"{name}:device:swap{swap_every}:T{T2}", ch4.trace(), ch4.collect(), ref2, noise2, T2, lib, check_U=True)
        _assert_tempering_state(ch4, ref2, f"{name} T={T2}")
        ch4.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 4. the law
_KERNELS = {}


def _kernels(name, case, betas):
    if name not in _KERNELS:
        _KERNELS[name] = (case,) + ht.kernels_of(case, betas, 2)
    return _KERNELS[name]


def _ensembles_against(label, m, c, betas, swap_every, n_ens, T, start_rows, expected, states, index, **kw):
    R, S = len(betas), states.shape[0]
    x0 = np.tile(np.stack([states[s].numpy().astype(np.uint8) for s in start_rows]), (n_ens, 1))
    ch = _chains(m, c, n_ens * R, T, 2, c["nmut"], 1, c["allowed"], betas, swap_every, x0=x0, random_chain=-1, **kw)
    ch.run(T)
    ch.sync()
    idx, st = ch.peek()["idx"], ch.tempering_state()
    ch.close()
    cells, forbidden = ht.joint_cells(idx, st["rung"], R, c["allowed"], index, states[start_rows[0]].numpy(), S)
    assert forbidden == 0
    chi2, df = hl.chi_square(np.bincount(cells, minlength=S ** R).astype(np.float64), n_ens * expected)
    print(f"tempering law, {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f}); "
          f"swaps {st['swap_accepts'].sum()} / {st['swap_attempts'].sum()}")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)
    return st


def test_law_of_two_rungs_with_exchange():
    """Case A, 2^16 ensembles (131 072 chains), beta = (1, 1/2), a swap event behind every iteration: T = 1 from the wild type and
    from the joint start state the CPU power test picked, T = 2 from the latter on both gradient policies, T = 12."""
    c, Ks, states, index, E, _ = _kernels("A", ht.case_a(), ht.BETAS_A)
    m = hl.hip_model_of(c)
    n_ens = 1 << 16
    wt_row = index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]
    other = ht.POWER_START_A
    for T, start in ((1, (wt_row, wt_row)), (1, other), (2, other), (12, (wt_row, wt_row))):
        expected = ht.joint_law(T, Ks, E, ht.BETAS_A, 1, start[0] * 35 + start[1])
        for reuse in ((True, False) if T == 2 else (True,)):
            st = _ensembles_against(f"case A: T={T} start={start} reuse={reuse}", m, c, ht.BETAS_A, 1, n_ens, T, start, expected, states,
                                    index, seed=1977 + 13 * T + start[0], reuse_grad=reuse)
            assert st["swap_attempts"].sum() == n_ens * ((T + 1) // 2)                       # the odd events have no pair
    m.close()


def test_law_of_four_rungs_with_exchange_every_second_iteration():
    """Case B, 2^15 ensembles, beta = (1, 1/2, 1/4, 1/8), swap_every 2: T = 2 (one even event), 3 (and an iteration without), 8
    (both parities twice)."""
    c, Ks, states, index, E, _ = _kernels("B", ht.case_b(), ht.BETAS_B)
    m = hl.hip_model_of(c)
    n_ens = 1 << 15
    for T, start in ((2, (0, 0, 0, 0)), (3, (4, 1, 3, 2)), (8, (0, 0, 0, 0))):
        j0 = int(np.ravel_multi_index(start, (5,) * 4))
        expected = ht.joint_law(T, Ks, E, ht.BETAS_B, ht.SWAP_EVERY_B, j0)
        _ensembles_against(f"case B: T={T} start={start}", m, c, ht.BETAS_B, ht.SWAP_EVERY_B, n_ens, T, start, expected, states, index,
                           seed=2977 + T)
    m.close()


@pytest.mark.parametrize("L,Lp,i0,site", [(104, 6, 98, 101), (237, 6, 200, 203)])
def test_law_in_the_two_and_three_groups_per_thread_forms(L, Lp, i0, site):
    c, Ks, states, index, E, _ = _kernels(f"L{L}", ht.one_site_case(L, Lp, i0, site), ht.BETAS_A)
    assert (L * 5 + 511) // 512 == {104: 2, 237: 3}[L]
    m = hl.hip_model_of(c)
    S = states.shape[0]
    for T, start in ((1, (3, 11)), (2, (3, 11))):
        expected = ht.joint_law(T, Ks, E, ht.BETAS_A, 1, start[0] * S + start[1])
        _ensembles_against(f"L={L}: T={T}", m, c, ht.BETAS_A, 1, 1 << 15, T, start, expected, states, index, seed=3977 + T)
    m.close()


# ------------------------------------------------------------------------------------------------ 5. equilibrium
def test_the_ensembles_reach_the_product_law():
    """After 64 iterations from the wild type the ensembles ARE a sample of prod_r exp(beta_r E)/Z_r (the enumerated K^64 row is
    within 1e-6 of it in total variation, asserted first on the CPU)."""
    c, Ks, states, index, E, _ = _kernels("A", ht.case_a(), ht.BETAS_A)
    pi = ht.product_law(E, ht.BETAS_A)
    wt_row = index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]
    T = 64
    assert hr.total_variation(ht.joint_law(T, Ks, E, ht.BETAS_A, 1, wt_row * 35 + wt_row), pi) <= 1e-6
    m = hl.hip_model_of(c)
    _ensembles_against("equilibrium against the product law, T=64", m, c, ht.BETAS_A, 1, 1 << 16, T, (wt_row, wt_row), pi, states, index,
                       seed=4713)
    m.close()


# ------------------------------------------------------------------------------------------------ 6. sharding
def test_sharding_does_not_change_a_tempering_run(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    T, lo, hi = 25, c["i0"], c["i0"] + c["Lp"] - 1

    def run(n_, off):
        ch = _chains(m, c, n_, T, 2, 3, 1, lib, ht.REPLAY_BETAS, 1, lo=lo, hi=hi, chain_offset=off, random_chain=0 if off == 0 else -1)
        ch.run(T)
        r, st, h = ch.collect(), ch.tempering_state(), ch.tempering_history()
        ch.close()
        return r, st, h

    (one, st1, h1), (a, sta, ha), (b, stb, hb) = run(16, 0), run(8, 0), run(8, 8)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    assert np.array_equal(np.concatenate([ha, hb], 1), h1) and (h1[-1] != h1[0]).any()
    for k in ("rung", "beta", "swap_attempts", "swap_accepts"):
        assert np.array_equal(np.concatenate([sta[k], stb[k]], 0), st1[k]), k
    assert 0 < st1["swap_accepts"].sum() < st1["swap_attempts"].sum()
    for n_, off, what in ((8, 6, "chain_offset"), (14, 0, "n_chains")):
        ch = Chains(m, n_, T, 2, 3, False, lo, hi, 3, 1, seed=99, chain_offset=off)
        ch.set_reversible(True)
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what} must be a multiple"):
            ch.set_tempering(ht.REPLAY_BETAS, 1)
        ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 7. the C ABI
def test_set_tempering_refusals(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    n, T = 8, 20
    ch = Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*needs reversible mode"):
        ch.set_tempering((1.0, 0.5))
    ch.set_reversible(True)
    for bad, what in (((1.0, 1.0), "strictly decreasing"), ((0.5, 1.0), "strictly decreasing"), ((1.0, 0.0), "finite and positive"),
                      ((1.0, -1.0), "finite and positive"), ((1.0, float("nan")), "finite and positive"),
                      ((float("inf"), 1.0), "finite and positive"), (tuple(2.0 - 0.01 * i for i in range(65)), r"1\.\.64"),
                      ((1.0, 0.5, 0.25), "n_chains must be a multiple")):
        with pytest.raises(PpdeHipError, match=rf"\[-1\].*{what}"):
            ch.set_tempering(bad)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*negative swap_every"):
        ch.set_tempering((1.0, 0.5), -1)
    ch.set_tempering((1.0, 0.5), 1)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*tempering is set and needs reversible mode"):
        ch.set_reversible(False)
    ch.set_tempering(None)                                                                   # cleared: the mode may go again
    ch.set_reversible(False)
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no tempering was set"):
        ch.tempering_state()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no tempering was set"):
        ch.tempering_history()
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_tempering((1.0, 0.5))
    ch.close()
    ch = Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7, n_streams=2)
    ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_tempering((1.0, 0.5))
    ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 8. PPDE_PAS
def test_ppde_pas_runs_the_chains_a_caller_would_build_by_hand():
    import argparse
    import contextlib
    import io
    import os
    import tempfile
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    betas = (1.0, 0.7, 0.5, 0.35)
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True, ppde_betas=betas, ppde_swap_every=2)
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
        ch.set_tempering(betas, 2)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res, st, hist = ch.collect(), ch.tempering_state(), ch.tempering_history()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(f_hist, res["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"]) and np.array_equal(best_e, res["best_energy"])
        assert np.array_equal(np.stack([r.argmax(-1) for r in rtraj]), res["random_traj"])
        tp = sampler.tempering
        assert np.array_equal(tp["betas"], np.asarray(betas, np.float32)) and np.array_equal(tp["rung_history"], hist)
        assert tp["rung_history"].shape == (T + 1, n)
        assert np.array_equal(tp["swap_attempts"], st["swap_attempts"]) and np.array_equal(tp["swap_accepts"], st["swap_accepts"])
        assert st["swap_attempts"].sum() == (n // 4) * (5 * 2 + 5 * 1)                       # ten events: five of two pairs, five of one
        assert f"   # swaps accepted = {int(st['swap_accepts'].sum())} / {int(st['swap_attempts'].sum())}" in buf.getvalue()
        assert (e_hist[1:] != e_hist[:-1]).any()

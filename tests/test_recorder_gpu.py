"""The recorder on the GPU (ppde_chains_set_recorder; k_record in ppde_amd/csrc/record.h): a recorded row is the peek of a twin
run stepped one iteration at a time, bit for bit, in every mode, under both gradient policies, from graphs and eagerly, and the
recording run's results are the twin's; with a ladder the slot follows its rung through the swaps; site counts are the bincount
of the stored samples at every layout edge; the recorded rows follow the enumerated law; the interfaces around it.

Everything but the law tests is exact (array_equal, floats compared as bits). The law tests use tests/test_reversible_gpu.py's
statistic and bound unchanged (helpers_library.chi_square, chi_square_bound, state_cells); tests/test_recorder_cpu.py asserts
the conditions they stand on (a recorder reading the slot before the swap, or the wrong rung, would land far outside)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht
from ppde_amd import library as dl
from ppde_amd import synthetic

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
N, T_LONG, PAS, NMUT, SEED = 16, 130, 2, 3, 202           # 130 = one 100 segment, one 20 segment and 10 eager steps
BETAS = ht.REPLAY_BETAS
MODES = ("default", "library", "reversible", "tempering")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _make(m, c, lib, mode, n, T, rng_mode=1, reuse=True, swap_every=1, recorder=None, x0=None, lo=None, hi=None, nmut=NMUT,
          betas=BETAS, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", SEED)
    lo = c["i0"] if lo is None else lo
    hi = c["i0"] + c["Lp"] - 1 if hi is None else hi
    ch = Chains(m, n, T, PAS, nmut, False, lo, hi, 3 if c.get("cnn") is not None else 1, rng_mode, reuse_grad=reuse, **kw)
    if mode != "default":
        ch.set_library(lib)
    if mode in ("reversible", "tempering"):
        ch.set_reversible(True)
    if mode == "tempering":
        ch.set_tempering(betas, swap_every)
    if recorder is not None:
        ch.set_recorder(**recorder)
    x0 = np.tile(c["wt"], (n, 1)) if x0 is None else x0
    ch.init(torch.as_tensor(x0).cuda())
    return ch


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, m
    m.close()


_TWINS = {}


def _noise(c, T):
    import ppde_oracle as orc
    gen = torch.Generator().manual_seed(77)
    return [orc.draw_noise_torch(N, c["L"] * 20, PAS, generator=gen) for _ in range(T)]


def _feed(ch, noise):
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _twin(toy, mode, reuse, swap_every=1, rng_mode=1, T=T_LONG):
    """The run WITHOUT a recorder, stepped one iteration at a time and peeked after each: computed once per configuration."""
    key = (mode, reuse, swap_every if mode == "tempering" else None, rng_mode, T)
    if key not in _TWINS:
        c, lib, m = toy
        ch = _make(m, c, lib, mode, N, T, rng_mode, reuse, swap_every, trace=True)
        noise = _noise(c, T) if rng_mode == 0 else None
        peeks = [ch.peek()]
        for t in range(T):
            if rng_mode == 0:
                _feed(ch, noise[t:t + 1])
            else:
                ch.run(1)
            peeks.append(ch.peek())
        _TWINS[key] = dict(peeks=peeks, res=ch.collect(), tr=ch.trace(),
                           hist=ch.tempering_history() if mode == "tempering" else None)
        ch.close()
    return _TWINS[key]


def _recording_run(toy, mode, reuse, recorder, swap_every=1, rng_mode=1, T=T_LONG):
    c, lib, m = toy
    ch = _make(m, c, lib, mode, N, T, rng_mode, reuse, swap_every, recorder=recorder, trace=True)
    if rng_mode == 0:
        _feed(ch, _noise(c, T))
    else:
        ch.run(T)
        gs = ch.graph_stats()
        assert (gs["replayed_steps"], gs["eager_steps"]) == ((T // 20) * 20, T % 20)       # graphs and eager issue both ran
    out = dict(rec=ch.recorded(), res=ch.collect(), tr=ch.trace(), shape=ch.recorder_shape(),
               hist=ch.tempering_history() if mode == "tempering" else None)
    ch.close()
    return out


def _assert_rows_are_peeks(rec, peeks, burn_in, every, T, label):
    rows = (T - burn_in) // every
    assert rec["rows"] == rows and rec["idx"].shape[0] == rows, label
    for s in range(rows):
        pk, chain = peeks[burn_in + (s + 1) * every], rec["chain"][s]
        assert np.array_equal(rec["idx"][s], pk["idx"][chain]), (label, s)
        assert np.array_equal(_bits(rec["energy"][s]), _bits(pk["energy"][chain])), (label, s)
        assert np.array_equal(_bits(rec["fitness"][s]), _bits(pk["fitness"][chain])), (label, s)


def _assert_counts_are_the_bincount(rec, label=""):
    idx = rec["idx"]
    L = idx.shape[2]
    want = np.stack([np.bincount(idx[:, :, l].ravel(), minlength=20) for l in range(L)]).astype(np.uint64)
    assert np.array_equal(rec["site_counts"], want), label


def _assert_nothing_else_changed(out, twin, label):
    for k in RESULT_KEYS:
        assert np.array_equal(out["res"][k], twin["res"][k]), (label, k)
    for k in TRACE_KEYS:
        assert np.array_equal(out["tr"][k], twin["tr"][k]), (label, k)


# ------------------------------------------------------------------------------------------------ 1. a row is a peek
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_a_recorded_row_is_the_peek_after_that_iteration(toy, mode, reuse):
    """TOY24, 16 chains, pas_length 2, nmut_threshold 3, T = 130 on the device RNG, recorders (burn_in, every) = (0, 1), (3, 4)."""
    c, _, _ = toy
    twin = _twin(toy, mode, reuse)
    for burn_in, every in ((0, 1), (3, 4)):
        label = f"{mode} reuse={reuse} burn_in={burn_in} every={every}"
        out = _recording_run(toy, mode, reuse, dict(every=every, burn_in=burn_in))
        rec = out["rec"]
        assert out["shape"] == ((T_LONG - burn_in) // every,) * 2 + (N,)
        assert rec["idx"].shape == (rec["rows"], N, c["L"]) and rec["energy"].dtype == np.float32 and rec["chain"].dtype == np.int32
        assert (rec["chain"] == np.arange(N)[None]).all(), label
        _assert_rows_are_peeks(rec, twin["peeks"], burn_in, every, T_LONG, label)
        _assert_counts_are_the_bincount(rec, label)
        _assert_nothing_else_changed(out, twin, label)
        if mode == "tempering":
            assert np.array_equal(out["hist"], twin["hist"])
        if mode == "default" and every == 1:
            # the rows hold the POST-reset state: rebuild the pre-reset one (the accepted proposal) from the trace
            tr, prev, resets = out["tr"], np.tile(c["wt"], (N, 1)), 0
            for t in range(T_LONG):
                pre = prev.copy()
                for b in np.flatnonzero(tr["accepted"][t]):
                    for s in range(int(tr["U"][t, b])):
                        l, k = divmod(int(tr["flat"][t, s, b]), 20)
                        pre[b, l] = k
                differs = (pre != rec["idx"][t]).any(1)
                assert (rec["idx"][t][differs] == c["wt"][None]).all()                      # ... and a reset goes to the wild type
                resets += int(differs.sum())
                prev = rec["idx"][t]
            assert resets > 0, "no mutation-cap reset in this run: the post-reset reading is not exercised"
    assert twin["tr"]["accepted"].any() and not twin["tr"]["accepted"].all()


def test_a_recorded_row_is_the_peek_on_caller_supplied_noise(toy):
    """rng_mode 0 (every iteration its own eager launch sequence), T = 12, every mode."""
    T = 12
    for mode in MODES:
        twin = _twin(toy, mode, True, rng_mode=0, T=T)
        for burn_in, every in ((0, 1), (3, 4)):
            out = _recording_run(toy, mode, True, dict(every=every, burn_in=burn_in), rng_mode=0, T=T)
            _assert_rows_are_peeks(out["rec"], twin["peeks"], burn_in, every, T, f"{mode} rng_mode 0")
            _assert_counts_are_the_bincount(out["rec"])
            _assert_nothing_else_changed(out, twin, f"{mode} rng_mode 0")


# ------------------------------------------------------------------------------------------------ 2. rung following
@pytest.mark.parametrize("swap_every", [0, 1, 5])
def test_the_slot_follows_its_rung_through_the_swaps(toy, swap_every):
    R = len(BETAS)
    for reuse in ((True, False) if swap_every == 1 else (True,)):
        twin = _twin(toy, "tempering", reuse, swap_every)
        for rung in (0, R - 1):
            for burn_in, every in ((0, 1), (3, 4)):
                label = f"swap_every={swap_every} rung={rung} reuse={reuse} ({burn_in}, {every})"
                out = _recording_run(toy, "tempering", reuse, dict(every=every, burn_in=burn_in, rung=rung), swap_every)
                rec = out["rec"]
                assert rec["chain"].shape == (rec["rows"], N // R) and out["shape"][2] == N // R
                assert np.array_equal(out["hist"], twin["hist"])
                for s in range(rec["rows"]):
                    t = burn_in + (s + 1) * every
                    holder = np.argmax(twin["hist"][t].reshape(N // R, R) == rung, 1) + np.arange(N // R) * R
                    assert (twin["hist"][t][holder] == rung).all()
                    assert np.array_equal(rec["chain"][s], holder), (label, s)
                _assert_rows_are_peeks(rec, twin["peeks"], burn_in, every, T_LONG, label)
                _assert_counts_are_the_bincount(rec, label)
                _assert_nothing_else_changed(out, twin, label)
                start = np.arange(N // R) * R + rung
                if swap_every == 0:
                    assert (rec["chain"] == start[None]).all()
                else:
                    assert (rec["chain"] != start[None]).any(), "no accepted swap moved the slot: nothing was followed"
                    assert (np.diff(rec["chain"], axis=0) != 0).any()


# ------------------------------------------------------------------------------------------------ 3. layout edges
@pytest.mark.parametrize("L,Lp,i0,site", [(8, 6, 1, 4), (70, 6, 62, 66), (104, 6, 98, 101), (237, 6, 200, 203)])
def test_site_counts_at_the_layout_edges(L, Lp, i0, site):
    """Potts-only one-site geometries (state rows of 5 to 61 dwords, always an odd number: the last workgroup owns a ragged piece), populations on
    both sides of a wave and of a workgroup's first pass, every = 1, T = 6."""
    from ppde_amd import _hip
    c = ht.one_site_case(L, Lp, i0, site)
    m = hl.hip_model_of(c)
    T = 6
    for n in (1, 63, 64, 65, 130):
        recs = []
        for keep in (True, False):
            ch = _make(m, c, c["allowed"], "reversible", n, T, recorder=dict(every=1, keep_samples=keep), lo=0, hi=L - 1, nmut=0,
                       seed=500 + n, random_chain=-1)
            ch.run(T)
            recs.append(ch.recorded())
            if not keep:
                buf = np.empty((1, n, L), np.uint8)
                with pytest.raises(_hip.PpdeHipError, match=r"\[-1\].*site counts only"):
                    _hip.check(ch.lib.ppde_chains_recorder_read(ch.handle, 0, 1, _hip.ptr(buf), None, None, None, None))
            ch.close()
        rec, counts_only = recs
        assert rec["rows"] == T and rec["idx"].shape == (T, n, L)
        _assert_counts_are_the_bincount(rec, f"L={L} n={n}")
        assert (rec["site_counts"].sum(1) == T * n).all()
        frozen = np.setdiff1d(np.arange(L), [site])
        assert (rec["site_counts"][frozen, c["wt"][frozen]] == T * n).all()
        assert counts_only["idx"] is None and np.array_equal(counts_only["site_counts"], rec["site_counts"])
        if n >= 63:
            assert (rec["site_counts"][site] > 0).sum() > 1                                  # the open residue moved
    m.close()


# ------------------------------------------------------------------------------------------------ 4. the law
def _chi2_of_row(label, idx_row, c, states, index, start_state, expected):
    cells, forbidden = hl.state_cells(idx_row, c["allowed"], index, start_state)
    assert forbidden == 0
    chi2, df = hl.chi_square(np.bincount(cells, minlength=states.shape[0]).astype(np.float64), idx_row.shape[0] * expected)
    print(f"recorder law, {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)


def test_law_of_the_recorded_rows_of_one_reversible_run():
    """law_case(), 2^16 reversible chains, T = 12, every = 1: the rows after 1, 2 and 12 iterations of ONE run against K^t."""
    from test_reversible_gpu import _law
    c, K, states, index, _, _ = _law("two residues, 7 and 5 letters, paths of 1-3 moves")
    m = hl.hip_model_of(c)
    n, T = 1 << 16, 12
    start = index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]
    ch = _make(m, c, c["allowed"], "reversible", n, T, recorder=dict(every=1), lo=0, hi=c["L"] - 1, nmut=c["nmut"], seed=6011,
               random_chain=-1)
    ch.run(T)
    assert ch.recorder_shape() == (T, T, n)
    for t in (1, 2, 12):
        row = ch.recorded(first=t - 1, count=1)["idx"][0]
        _chi2_of_row(f"reversible, t={t}", row, c, states, index, states[start].numpy(), np.linalg.matrix_power(K, t)[start])
    ch.close()
    m.close()


def test_law_of_the_recorded_rung_of_a_tempering_run():
    """case_a(), beta = (1, 1/2), 2^16 ensembles from the joint start (17, 3), a swap behind every iteration, the recorder on
    rung 0: the row after one iteration against rung 0's marginal of the joint law (a recorder that read the slot before the
    swap scores 299 701 there, tests/test_recorder_cpu.py), the row after 64 against exp(E)/Z."""
    from test_tempering_gpu import _kernels
    c, Ks, states, index, E, inside = _kernels("A", ht.case_a(), ht.BETAS_A)
    S = states.shape[0]
    m = hl.hip_model_of(c)
    n_ens, T, start = 1 << 16, 64, ht.POWER_START_A
    x0 = np.tile(np.stack([states[s].numpy().astype(np.uint8) for s in start]), (n_ens, 1))
    ch = _make(m, c, c["allowed"], "tempering", 2 * n_ens, T, recorder=dict(every=1, rung=0), x0=x0, lo=0, hi=c["L"] - 1,
               nmut=c["nmut"], betas=ht.BETAS_A, seed=6029, random_chain=-1)
    ch.run(T)
    first, last = ch.recorded(first=0, count=1), ch.recorded(first=T - 1, count=1)
    st = ch.tempering_state()
    ch.close()
    m.close()
    assert 0 < st["swap_accepts"].sum() < st["swap_attempts"].sum()
    assert (st["rung"][last["chain"][0]] == 0).all()                                         # the slot ends on the chain that holds rung 0
    marginal = ht.joint_law(1, Ks, E, ht.BETAS_A, 1, start[0] * S + start[1]).reshape(S, S).sum(1)
    _chi2_of_row("tempering, rung 0, t=1", first["idx"][0], c, states, index, states[start[0]].numpy(), marginal)
    _chi2_of_row("tempering, rung 0, t=64", last["idx"][0], c, states, index, states[start[0]].numpy(), hr.target_law(E, inside))


# ------------------------------------------------------------------------------------------------ 5. interfaces
def test_recorder_refusals_and_partial_reads(toy):
    from ppde_amd import _hip
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    n, T = 8, 130
    bad = pytest.raises
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no recorder was set"):
        ch.recorder_shape()
    for kw, what in ((dict(every=0), "every must be >= 1"), (dict(every=-2), "every must be >= 1"),
                     (dict(every=1, burn_in=-1), "negative burn_in"), (dict(every=1, burn_in=T), "no iteration"),
                     (dict(every=T + 1), "no iteration"), (dict(every=4, burn_in=T - 3), "no iteration"),
                     (dict(every=1, rung=-2), "rung must be -1"), (dict(every=1, rung=0), "needs tempering")):
        with bad(_hip.PpdeHipError, match=rf"\[-1\].*{what}"):
            ch.set_recorder(**kw)
    cfg = _hip.RecordConfig(burn_in=0, every=1, rung=-1, keep_samples=2)
    import ctypes
    with bad(_hip.PpdeHipError, match=r"\[-1\].*keep_samples must be 0 or 1"):
        _hip.check(ch.lib.ppde_chains_set_recorder(ch.handle, ctypes.byref(cfg)))
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no recorder was set"):                         # every refusal left the object unchanged
        ch.recorder_shape()
    ch.set_recorder(every=T, burn_in=0)                                                      # burn_in + every = max_steps: one row
    assert ch.recorder_shape() == (0, 1, n)
    ch.set_recorder(None)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no recorder was set"):
        ch.recorder_shape()
    ch.set_library(lib)
    ch.set_reversible(True)
    ch.set_tempering(BETAS, 1)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*rung beyond the ladder"):
        ch.set_recorder(every=1, rung=len(BETAS))
    ch.set_recorder(every=10, burn_in=5, rung=1)
    for args in ((None,), ((1.0, 0.5), 1)):                                                  # to clear or to replace
        with bad(_hip.PpdeHipError, match=r"\[-1\].*recorder that follows a rung"):
            ch.set_tempering(*args)
    assert ch.recorder_shape() == (0, 12, n // len(BETAS))
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_recorder(every=1)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_recorder(None)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*beyond those recorded"):
        ch.recorded(first=0, count=1)
    assert ch.recorded()["rows"] == 0 and ch.recorded()["idx"].shape == (0, 2, c["L"])
    # a partial run: 50 iterations hold rows for t = 15, 25, 35, 45; the next 80 complete the twelve
    ch.run(50)
    part = ch.recorded()
    assert part["rows"] == 4 and ch.recorder_shape()[0] == 4
    with bad(_hip.PpdeHipError, match=r"\[-1\].*beyond those recorded"):
        ch.recorded(first=0, count=5)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*beyond those recorded"):
        ch.recorded(first=-1, count=1)
    ch.run(80)
    full = ch.recorded()
    assert full["rows"] == 12
    for k in ("idx", "energy", "fitness", "chain"):
        assert np.array_equal(full[k][:4], part[k]), k
        assert np.array_equal(ch.recorded(first=7, count=3)[k], full[k][7:10]), k
    _assert_counts_are_the_bincount(full)
    _assert_counts_are_the_bincount(part)
    eh = ch.collect()["energy_history"]
    for s in range(12):
        assert np.array_equal(_bits(full["energy"][s]), _bits(eh[15 + 10 * s][full["chain"][s]]))
    assert ch.lib.ppde_chains_recorder_read(ch.handle, 0, 12, None, None, None, None, None) == 0   # any pointer may be NULL
    ch.close()
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7, n_streams=2)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_recorder(every=1)
    ch.close()


# ------------------------------------------------------------------------------------------------ 6. sharding, PPDE_PAS, driver
def test_sharding_does_not_change_what_is_recorded(toy):
    c, lib, m = toy
    T, R = 25, len(BETAS)

    def run(mode, n_, off, rung):
        ch = _make(m, c, lib, mode, n_, T, recorder=dict(every=2, burn_in=1, rung=rung), chain_offset=off, random_chain=-1, seed=99)
        ch.run(T)
        r = ch.recorded()
        ch.close()
        return r

    for mode, rung in (("default", None), ("reversible", None), ("tempering", 0), ("tempering", R - 1)):
        one, a, b = run(mode, 16, 0, rung), run(mode, 8, 0, rung), run(mode, 8, 8, rung)
        assert one["rows"] == 12
        for k in ("idx", "energy", "fitness"):
            assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), (mode, k)
        assert np.array_equal(np.concatenate([a["chain"], b["chain"] + 8], 1), one["chain"]), mode
        assert np.array_equal(a["site_counts"] + b["site_counts"], one["site_counts"]), mode


def test_ppde_pas_and_the_driver_hand_the_samples_out():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    L = len(seq)
    n, T, pas, nmut, seed = 8, 30, 2, 3, 4242
    betas = (1.0, 0.7, 0.5, 0.35)
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        base = dict(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n, device="cuda:0",
                    ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox", ppde_seed=seed)
        en = ProteinProductOfExperts(argparse.Namespace(**base))
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        for ladder in (False, True):
            extra = dict(ppde_reversible=True, ppde_betas=betas, ppde_swap_every=2) if ladder else {}
            runs = []
            for sample in (False, True):
                rec_args = dict(ppde_sample_every=4, ppde_sample_burn_in=2) if sample else {}
                np.random.seed(5)
                with contextlib.redirect_stdout(io.StringIO()):
                    sampler = PPDE_PAS(argparse.Namespace(**base, **extra, **rec_args))
                    runs.append(sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10))
                if not sample:
                    assert sampler.samples is None
            assert len(runs[1]) == 6                                                         # the returned tuple does not change
            assert torch.equal(runs[0][0], runs[1][0])
            for k in range(1, 5):
                assert np.array_equal(runs[0][k], runs[1][k]), k
            assert all(np.array_equal(a, b) for a, b in zip(runs[0][5], runs[1][5]))
            np.random.seed(5)
            lo_hi = (0, L - 1) if ladder else (i0, i0 + Lp - 1)
            ch = Chains(en.model, n, T, pas, nmut, False, *lo_hi, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
            if ladder:
                ch.set_library(dl.fold_range(dl.full_library(L), i0, i0 + Lp - 1))
                ch.set_reversible(True)
                ch.set_tempering(betas, 2)
            ch.set_recorder(4, 2, 0 if ladder else None)
            ch.init(en.model.onehot_to_idx(x0))
            ch.run(T)
            want = ch.recorded()
            ch.close()
            got = sampler.samples
            assert got["rows"] == want["rows"] == 7 and got["idx"].shape == (7, n // 4 if ladder else n, L)
            for k in ("idx", "energy", "fitness", "chain", "site_counts"):
                assert np.array_equal(got[k], want[k]), (ladder, k)
        # the driver: the listed files with these shapes, beside the existing ones
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_rec", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        common = ["--protein_weights", root, "--protein", "TOY24", "--results_path", res, "--device", "cuda:0",
                  "--disable_MSA_transformer_scoring", "--n_chains", "12", "--n_iters", "40", "--seed", "3", "--log_every", "25",
                  "--nmut_threshold", "4", "--ppde_rng", "philox", "--ppde_sample_every", "5", "--ppde_sample_burn_in", "10"]
        old = {"config.txt", "population.npy", "pred_fitness_scores.npy", "oracle_fitness_scores.npy", "potts_scores.npy",
               "energy_scores.npy", "energy_history.npy", "fitness_history.npy"}
        new = {"samples.npy": (6, 12, L), "sample_energy.npy": (6, 12), "sample_fitness.npy": (6, 12), "sample_chain.npy": (6, 12),
               "site_counts.npy": (L, 20)}
        args = drv.build_parser().parse_args(common + ["--run_signature", "plain"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))} == old | set(new)
        for f, shape in new.items():
            assert np.load(os.path.join(out, f)).shape == shape, f
        sm, eh = np.load(os.path.join(out, "samples.npy")), np.load(os.path.join(out, "energy_history.npy"))
        assert sm.dtype == np.uint8 and np.array_equal(np.load(os.path.join(out, "sample_energy.npy")), eh[15::5])
        assert np.load(os.path.join(out, "site_counts.npy")).sum() == 6 * 12 * L
        args = drv.build_parser().parse_args(common + ["--run_signature", "ladder", "--ppde_reversible", "--ppde_betas", "1,0.7,0.5",
                                                       "--ppde_swap_every", "2", "--ppde_sample_counts_only"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))} == \
            old | {"site_counts.npy", "rung_history.npy", "swap_attempts.npy", "swap_accepts.npy"}
        assert np.load(os.path.join(out, "rung_history.npy")).shape == (41, 12)
        assert np.load(os.path.join(out, "swap_attempts.npy")).shape == (4, 2) == np.load(os.path.join(out, "swap_accepts.npy")).shape
        assert np.load(os.path.join(out, "site_counts.npy")).sum() == 6 * 4 * L               # rung 0 of four ensembles

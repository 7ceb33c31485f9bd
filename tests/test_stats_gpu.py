"""The move statistics on the GPU (ppde_chains_set_stats; k_stats in ppde_amd/csrc/stats.h): the nine
counters equal the rule (helpers_stats.stats_of, the only reference) applied to a twin run -- the same run without statistics and
with trace = 1, stepped one iteration at a time and peeked after each --, exactly (array_equal on int64): in every mode, under both
gradient policies, from graphs and eagerly, on caller-supplied noise, under paper_results, at every layout edge of the state row; and
the results of the run with statistics are the twin's, bit for bit.

Each test asserts on its twin that the branch it means to check was taken (helpers_stats.events); tests/test_stats_cpu.py asserts the
same conditions on CPU reference runs of the toy configurations.

A clamp that actually shortens a supplied path cannot be observed: an iteration of caller-supplied noise whose max_u lies below a
supplied U is refused by the chain kernels themselves (ppde_chains_sync: PPDE_ERR_INVALID, "exceeds the max_u"), for the twin too, so
nothing can be read after it. The clamp by max_u is exercised with an iteration whose max_u (2) lies below mu_max (3) and whose
path lengths fit it, and the refusal is asserted with statistics as without."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_archive as ha
import helpers_library as hl
import helpers_reversible as hr
import helpers_stats as hs
import helpers_tempering as ht

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
N, T_LONG, PAS, NMUT, SEED = 16, 130, 2, 3, 202           # 130 = one 100 segment, one 20 segment and 10 eager steps
BETAS = ht.REPLAY_BETAS
MODES = ("default", "library", "reversible", "tempering")


def _assert_stats_equal(got, want, label, per_site=True):
    for k in hs.KEYS:
        if k == "site_changes" and not per_site:
            assert got[k] is None, label
            continue
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (label, k, got[k], want[k])


def _make(m, c, lib, mode, n, T, rng_mode=1, reuse=True, swap_every=1, stats=None, x0=None, lo=None, hi=None, nmut=NMUT,
          betas=BETAS, pas=PAS, paper=False, before=None, after=None, **kw):
    """stats: None (no statistics), True / False = per_site. `before` / `after`: callables that set other observers."""
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", SEED)
    lo = c["i0"] if lo is None else lo
    hi = c["i0"] + c["Lp"] - 1 if hi is None else hi
    ch = Chains(m, n, T, pas, nmut, paper, lo, hi, 3 if c.get("cnn") is not None else 1, rng_mode, reuse_grad=reuse, **kw)
    if mode != "default":
        ch.set_library(lib)
    if mode in ("reversible", "tempering"):
        ch.set_reversible(True)
    if mode == "tempering":
        ch.set_tempering(betas, swap_every)
    if before is not None:
        before(ch)
    if stats is not None:
        ch.set_stats(stats)
    if after is not None:
        after(ch)
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
    """Caller-supplied noise of T iterations; in iteration 1 every path length is at most 2 and the block holds 2 sub-steps, so that
    iteration's max_u lies below mu_max = 3."""
    import ppde_oracle as orc
    gen = torch.Generator().manual_seed(77)
    out = [orc.draw_noise_torch(N, c["L"] * 20, PAS, generator=gen) for _ in range(T)]
    U, q, u = out[1]
    out[1] = (U.clamp(max=2), q[:2].contiguous() if q.shape[0] >= 2 else q, u)
    return out


def _feed(ch, noise):
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _stepped(ch, T, noise=None):
    peeks = [ch.peek()]
    for t in range(T):
        if noise is not None:
            _feed(ch, noise[t:t + 1])
        else:
            ch.run(1)
        peeks.append(ch.peek())
    return peeks


def _twin(case, mode, reuse, rng_mode=1, T=T_LONG, n=N, **kw):
    """The run WITHOUT statistics, with trace = 1, stepped one iteration at a time and peeked after each: once per configuration."""
    key = (id(case[2]), mode, reuse, rng_mode, T, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _TWINS:
        c, lib, m = case
        ch = _make(m, c, lib, mode, n, T, rng_mode, reuse, trace=True, **kw)
        peeks = _stepped(ch, T, _noise(c, T) if rng_mode == 0 else None)
        tr = ch.trace()
        assert all(np.array_equal(peeks[t]["accepted"], tr["accepted"][t - 1]) for t in range(1, T + 1))   # peek's accept bit is the trace's
        _TWINS[key] = dict(peeks=peeks, res=ch.collect(), tr=tr, hist=ch.tempering_history() if mode == "tempering" else None)
        ch.close()
    return _TWINS[key]


def _want(twin, mode, pas=PAS, upto=None, betas=BETAS):
    T = len(twin["peeks"]) - 1 if upto is None else upto
    R = len(betas) if mode == "tempering" else 0
    return hs.stats_of(twin["peeks"][:T + 1], twin["tr"]["accepted"], twin["tr"]["U"], twin["hist"], R, 2 * pas - 1)


def _events(twin, mode, pas=PAS, betas=BETAS):
    return hs.events(twin["peeks"], twin["tr"]["accepted"], twin["tr"]["U"], twin["hist"], len(betas) if mode == "tempering" else 0,
                     2 * pas - 1)


def _stats_run(case, mode, reuse, rng_mode=1, T=T_LONG, n=N, per_site=True, graphs=True, **kw):
    c, lib, m = case
    ch = _make(m, c, lib, mode, n, T, rng_mode, reuse, stats=per_site, trace=True, **kw)
    if rng_mode == 0:
        _feed(ch, _noise(c, T))
    else:
        ch.run(T)
        gs = ch.graph_stats()
        if graphs:
            assert (gs["replayed_steps"], gs["eager_steps"]) == ((T // 20) * 20, T % 20)       # graphs and eager issue both ran
        else:
            assert (gs["captures"], gs["replayed_steps"], gs["eager_steps"]) == (0, 0, T)
        assert gs["captures_in_run"] == 0
    out = dict(st=ch.stats(), res=ch.collect(), tr=ch.trace(), hist=ch.tempering_history() if mode == "tempering" else None)
    ch.close()
    return out


def _assert_nothing_else_changed(out, twin, label):
    for k in RESULT_KEYS:
        assert np.array_equal(out["res"][k], twin["res"][k]), (label, k)
    for k in TRACE_KEYS:
        assert np.array_equal(np.ascontiguousarray(out["tr"][k]).view(np.uint8), np.ascontiguousarray(twin["tr"][k]).view(np.uint8)), (label, k)
    if twin["hist"] is not None:
        assert np.array_equal(out["hist"], twin["hist"]), label


# ------------------------------------------------------------------------------------------------ 1. the rule, every mode
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("mode,swap_every", [("default", 1), ("library", 1), ("reversible", 1), ("tempering", 1), ("tempering", 3)])
def test_the_statistics_are_the_rule_on_the_twin(toy, mode, swap_every, reuse):
    """TOY24, 16 chains, pas_length 2, nmut_threshold 3, T = 130 on the device RNG. Under gradient reuse the accept of an iteration
    is fused with the next propose (not in tempering): there ChainRec::Ucur already holds the next path."""
    c, lib, _ = toy
    twin = _twin(toy, mode, reuse, swap_every=swap_every)
    ev = _events(twin, mode)
    label = f"{mode} swap_every={swap_every} reuse={reuse}"
    print(label, ev)
    assert (ev["acc_by_len"] >= 1).all() and (ev["rej_by_len"] >= 1).all(), (label, ev)         # both outcomes at every path length
    assert ev["short_jumps"] + ev["still_accepts"] >= 1, (label, ev)                            # an accepted path with h < U
    assert ev["moved_without_accept"] == 0, (label, ev)
    if mode == "default":
        assert ev["wt_returns"] >= 1, (label, ev)
    if mode == "tempering":
        assert ev["rung_moves"] >= 1, (label, ev)                                               # the rung after the swap is not the one iterated on
    if mode != "default":
        frozen = np.flatnonzero(np.asarray(lib) == 0)
        assert not np.intersect1d(ev["changed_sites"], frozen).size, label
    # the next iteration's path length differs from this one's somewhere: reading the record after a fused launch would be wrong
    U = twin["tr"]["U"]
    assert (U[1:] != U[:-1]).any()
    want = _want(twin, mode)
    out = _stats_run(toy, mode, reuse, swap_every=swap_every)
    _assert_stats_equal(out["st"], want, label)
    hs.assert_identities(out["st"], T_LONG)
    _assert_nothing_else_changed(out, twin, label)


# ------------------------------------------------------------------------------------------------ 2. caller-supplied noise
@pytest.mark.parametrize("mode", ["default", "reversible"])
def test_the_statistics_on_caller_supplied_noise(toy, mode):
    """rng_mode 0, fed iteration by iteration, T = 12; iteration 1 has max_u = 2 < mu_max."""
    T = 12
    twin = _twin(toy, mode, True, rng_mode=0, T=T)
    assert twin["tr"]["U"][1].max() <= 2 and twin["tr"]["U"].max() == 3
    out = _stats_run(toy, mode, True, rng_mode=0, T=T)
    _assert_stats_equal(out["st"], _want(twin, mode), f"{mode} rng_mode 0")
    hs.assert_identities(out["st"], T)
    _assert_nothing_else_changed(out, twin, f"{mode} rng_mode 0")


def test_a_path_length_beyond_its_noise_block_is_refused_with_statistics_as_without(toy):
    from ppde_amd import _hip
    c, lib, m = toy
    U, q, u = _noise(c, 2)[0]
    assert int(U.max()) == 3
    for stats in (None, True):
        ch = _make(m, c, lib, "default", N, 4, 0, True, stats=stats)
        with pytest.raises(_hip.PpdeHipError, match="exceeds the max_u"):
            ch.run(1, (U.to(torch.int32).reshape(1, -1), q[:2].contiguous(), u.reshape(1, -1), [2]))
        ch.close()


# ------------------------------------------------------------------------------------------------ 3. eager issue
def test_eager_issue_counts_what_graph_replay_counts(toy):
    for mode in ("default", "tempering"):
        twin = _twin(toy, mode, True)
        out = _stats_run(toy, mode, True, graphs=False, use_graph=False)
        _assert_stats_equal(out["st"], _want(twin, mode), f"{mode} eager")
        _assert_nothing_else_changed(out, twin, f"{mode} eager")


# ------------------------------------------------------------------------------------------------ 4. paper_results
@pytest.mark.parametrize("reuse", [True, False])
def test_under_paper_results_a_rejected_chain_moves(toy, reuse):
    """A start away from the wild type: a rejected chain falls back to its initial state, so it moves without an acceptance."""
    c, lib, m = toy
    x0 = np.tile(c["wt"], (N, 1))
    for b in range(N):
        x0[b, c["i0"] + b % c["Lp"]] = (x0[b, c["i0"] + b % c["Lp"]] + 1 + b % 3) % 20
    kw = dict(paper=True, x0=x0, nmut=0)
    twin = _twin(toy, "default", reuse, T=60, **kw)
    ev, want = _events(twin, "default"), _want(twin, "default")
    print("paper_results", ev)
    assert ev["moved_without_accept"] >= 1 and (want["moved"] > want["accepts"]).any()
    out = _stats_run(toy, "default", reuse, T=60, **kw)
    _assert_stats_equal(out["st"], want, f"paper_results reuse={reuse}")
    hs.assert_identities(out["st"], 60, paper=True)
    _assert_nothing_else_changed(out, twin, f"paper_results reuse={reuse}")


# ------------------------------------------------------------------------------------------------ 5. layout edges
@pytest.mark.parametrize("L", ha.EDGE_LENGTHS)
def test_the_statistics_at_the_layout_edges(L):
    """helpers_archive.edge_case: state rows of 5 to 79 dwords, open residues at both ends of the row and astride a dword boundary;
    5 chains, 40 iterations, reversible mode over the full range. Only open residues ever change: a counted pad byte would show as
    a jump_sum beyond the site counts or a mismatch with the rule."""
    c, lib, sites = ha.edge_case(L)
    m = hl.hip_model_of(c)
    case = (c, lib, m)
    kw = dict(lo=0, hi=L - 1, nmut=0, seed=705, random_chain=-1)
    twin = _twin(case, "reversible", True, T=40, n=5, **kw)
    ev = _events(twin, "reversible")
    assert set(ev["changed_sites"].tolist()) <= set(sites) and {0, L - 1} & set(ev["changed_sites"].tolist()), (L, ev)
    out = _stats_run(case, "reversible", True, T=40, n=5, **kw)
    _assert_stats_equal(out["st"], _want(twin, "reversible"), f"L={L}")
    hs.assert_identities(out["st"], 40)
    frozen = np.setdiff1d(np.arange(L), sites)
    assert (out["st"]["site_changes"][:, frozen] == 0).all()
    for key in [k for k in _TWINS if k[0] == id(m)]:
        del _TWINS[key]
    m.close()


# ------------------------------------------------------------------------------------------------ 6. chain counts
@pytest.mark.parametrize("n", [5, 65])
def test_a_ragged_last_wave_and_a_ragged_last_workgroup(toy, n):
    twin = _twin(toy, "default", True, T=40, n=n)
    out = _stats_run(toy, "default", True, T=40, n=n)
    _assert_stats_equal(out["st"], _want(twin, "default"), f"n={n}")
    hs.assert_identities(out["st"], 40)
    _assert_nothing_else_changed(out, twin, f"n={n}")


def test_a_ladder_over_a_population_of_many_ensembles(toy):
    n = 68                                                                                       # 17 ensembles of 4: more than one workgroup
    twin = _twin(toy, "tempering", True, T=40, n=n)
    out = _stats_run(toy, "tempering", True, T=40, n=n)
    _assert_stats_equal(out["st"], _want(twin, "tempering"), "n=68 tempering")
    hs.assert_identities(out["st"], 40)


# ------------------------------------------------------------------------------------------------ 7. path lengths
@pytest.mark.parametrize("pas", [1, 5])
def test_the_shapes_and_contents_of_the_length_counters(toy, pas):
    M = 2 * pas - 1
    for mode in ("default", "tempering"):
        twin = _twin(toy, mode, True, T=40, pas=pas, nmut=0 if pas == 5 else NMUT)
        out = _stats_run(toy, mode, True, T=40, pas=pas, nmut=0 if pas == 5 else NMUT)
        R = len(BETAS) if mode == "tempering" else 1
        assert out["st"]["len_attempts"].shape == (R, M) and out["st"]["len_accepts"].shape == (R, M)
        want = _want(twin, mode, pas=pas)
        assert (want["len_attempts"].sum(0) >= 1).all()                                          # every length was drawn
        _assert_stats_equal(out["st"], want, f"pas={pas} {mode}")
        hs.assert_identities(out["st"], 40)
        _assert_nothing_else_changed(out, twin, f"pas={pas} {mode}")


# ------------------------------------------------------------------------------------------------ 8. next to the other observers
@pytest.mark.parametrize("mode", ["default", "tempering"])
def test_every_observer_next_to_the_statistics_holds_what_it_holds_alone(toy, mode):
    c, lib, m = toy
    T, K = 40, 3

    def others(ch):
        ch.set_recorder(every=3, burn_in=2)
        ch.set_pair_counts(None)
        ch.set_archive(K)

    def run(**kw):
        ch = _make(m, c, lib, mode, N, T, **kw)
        ch.run(T)
        obs = "before" in kw or "after" in kw
        out = dict(rec=ch.recorded() if obs else None, pairs=ch.pair_counts() if obs else None, arc=ch.archive() if obs else None,
                   st=ch.stats() if kw.get("stats") is not None else None, res=ch.collect())
        ch.close()
        return out

    plain, only = run(before=others), run(stats=True)
    for order in ("before", "after"):
        both = run(stats=True, **{order: others})
        for k in ("idx", "energy", "fitness", "chain", "site_counts"):
            assert np.array_equal(both["rec"][k], plain["rec"][k]), (mode, order, k)
        assert np.array_equal(both["pairs"][0], plain["pairs"][0])
        for k in ("idx", "energy", "fitness", "step", "count"):
            assert np.array_equal(both["arc"][k].view(np.uint8), plain["arc"][k].view(np.uint8)), (mode, order, k)
        _assert_stats_equal(both["st"], only["st"], f"{mode} {order}")
        for k in RESULT_KEYS:
            assert np.array_equal(both["res"][k], plain["res"][k]), (mode, order, k)


# ------------------------------------------------------------------------------------------------ 9. reads across runs
def test_reads_across_runs_and_a_second_init(toy):
    c, lib, m = toy
    twin = _twin(toy, "default", True)
    ch = _make(m, c, lib, "default", N, T_LONG, stats=True)
    zero = ch.stats()
    assert all((zero[k] == 0).all() for k in hs.KEYS)                                            # before any run
    ch.run(50)
    _assert_stats_equal(ch.stats(), _want(twin, "default", upto=50), "after 50")
    ch.run(80)
    _assert_stats_equal(ch.stats(), _want(twin, "default"), "after 130")
    ch.init(torch.as_tensor(np.tile(c["wt"], (N, 1))).cuda())                                   # a second init zeroes everything
    zero = ch.stats()
    assert all((zero[k] == 0).all() for k in hs.KEYS)
    ch.run(50)
    _assert_stats_equal(ch.stats(), _want(twin, "default", upto=50), "after a second init")
    ch.close()


# ------------------------------------------------------------------------------------------------ 10. interfaces
def test_stats_refusals_null_pointers_and_no_sites(toy):
    from ppde_amd import _hip
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    n, T = 8, 40
    bad = pytest.raises
    nine = [None] * 9
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no statistics were set"):
        ch.stats()
    assert ch.lib.ppde_chains_stats_read(ch.handle, *nine) == -1
    for v in (2, -1, 7):
        cfg = _hip.StatsConfig(per_site=v)
        assert ch.lib.ppde_chains_set_stats(ch.handle, ctypes.byref(cfg)) == -1
        assert b"per_site must be 0 or 1" in ch.lib.ppde_last_error()
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no statistics were set"):                      # every refusal left the object unchanged
        ch.stats()
    ch.set_stats(True)
    ch.set_stats(None)                                                                          # cleared
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no statistics were set"):
        ch.stats()
    ch.set_stats(True)
    ch.set_stats(False)                                                                         # replaced: no per-site counts
    with bad(_hip.PpdeHipError, match=r"\[-1\].*not initialised"):
        ch.stats()
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_stats(True)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_stats(None)
    ch.run(30)
    st = ch.stats()
    assert st["site_changes"] is None and (st["iters"] == 30).all()
    sites = np.zeros((1, c["L"]), np.int64)
    assert ch.lib.ppde_chains_stats_read(ch.handle, *nine[:8], _hip.ptr(sites)) == -1            # site_changes without per_site
    assert b"per_site = 0" in ch.lib.ppde_last_error()
    assert ch.lib.ppde_chains_stats_read(ch.handle, *nine) == 0                                  # any pointer may be NULL
    R, M, ps = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _hip.check(ch.lib.ppde_chains_stats_shape(ch.handle, ctypes.byref(R), ctypes.byref(M), ctypes.byref(ps)))
    assert (R.value, M.value, ps.value) == (1, 3, 0) and ch.lib.ppde_chains_stats_shape(ch.handle, None, None, None) == 0
    # the same run with per-site counts: the other eight counters are the same
    full = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    full.set_stats(True)
    full.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    full.run(30)
    fs = full.stats()
    full.close()
    for k in hs.KEYS[:-1]:
        assert np.array_equal(fs[k], st[k]), k
    assert fs["site_changes"].sum() == fs["jump_sum"].sum() > 0
    ch.close()
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7, n_streams=2)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_stats(True)
    ch.close()
    # the ladder is fixed while statistics are set: neither cleared nor replaced
    ch = Chains(m, n, T, 2, 3, False, 0, c["L"] - 1, 3, 1, seed=7)
    ch.set_library(lib)
    ch.set_reversible(True)
    ch.set_tempering(BETAS, 1)
    ch.set_stats(True)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*move statistics are set"):
        ch.set_tempering(None)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*move statistics are set"):
        ch.set_tempering(BETAS[:2], 1)
    _hip.check(ch.lib.ppde_chains_stats_shape(ch.handle, ctypes.byref(R), ctypes.byref(M), ctypes.byref(ps)))
    assert (R.value, M.value, ps.value) == (4, 3, 1)
    ch.set_stats(None)
    ch.set_tempering(BETAS[:2], 1)                                                              # ... and free again once they are cleared
    ch.close()


# ------------------------------------------------------------------------------------------------ 11. sampler and driver
def test_ppde_pas_and_the_driver_hand_the_statistics_out():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import re
    import subprocess
    import sys
    import tempfile
    from ppde_amd import stats as chain_stats, synthetic
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    L = len(seq)
    n, T, pas, nmut, seed = 8, 30, 2, 3, 4242
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(repo, "scripts", "directed_evolution.py")
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res, tempfile.TemporaryDirectory() as res2:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        base = dict(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n, device="cuda:0",
                    ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox", ppde_seed=seed)
        en = ProteinProductOfExperts(argparse.Namespace(**base))
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        runs, logs = [], []
        for spec in (None, True, "no-sites"):
            np.random.seed(5)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                sampler = PPDE_PAS(argparse.Namespace(**base, ppde_stats=spec))
                runs.append(sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10))
            logs.append(buf.getvalue())
            if spec is None:
                assert sampler.stats is None
            elif spec is True:
                got = sampler.stats
            else:
                assert sampler.stats["site_changes"] is None and sampler.stats["summary"]["site_mobility"] is None
                for k in hs.KEYS[:-1]:
                    assert np.array_equal(sampler.stats[k], got[k]), k
        for r in runs[1:]:                                                                       # the returned tuple does not change
            assert len(r) == 6 and torch.equal(runs[0][0], r[0])
            for k in range(1, 5):
                assert np.array_equal(runs[0][k], r[k]), k
        line = r"   # acceptance so far = \d\.\d{3} \(path length 1: \d\.\d\d, 2: \d\.\d\d, 3: \d\.\d\d\)\n"
        assert len(re.findall(line, logs[1])) == 3 and "acceptance so far" not in logs[0]
        assert re.sub(line, "", logs[1]) == logs[0]                                              # the other lines are the default run's
        np.random.seed(5)
        ch = Chains(en.model, n, T, pas, nmut, False, i0, i0 + Lp - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_stats(True)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        want = ch.stats()
        ch.close()
        _assert_stats_equal({k: got[k] for k in hs.KEYS}, want, "PPDE_PAS")
        assert np.array_equal(got["chain"], np.arange(n)) and got["betas"] is None
        summ = chain_stats.summarise(want)
        assert set(got["summary"]) == set(summ)
        for k, v in summ.items():
            assert (v is None and got["summary"][k] is None) or np.array_equal(np.asarray(v), np.asarray(got["summary"][k]), equal_nan=True), k
        # the driver: the nine files beside the existing ones, and the same from two ranks
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_stats", script)
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        common = ["--protein_weights", root, "--protein", "TOY24", "--device", "cuda:0",
                  "--disable_MSA_transformer_scoring", "--n_chains", "13", "--n_iters", "40", "--seed", "3", "--log_every", "25",
                  "--nmut_threshold", "3", "--ppde_rng", "philox"]
        old = {"config.txt", "population.npy", "pred_fitness_scores.npy", "oracle_fitness_scores.npy", "potts_scores.npy",
               "energy_scores.npy", "energy_history.npy", "fitness_history.npy"}
        shapes = {f"stats_{k}.npy": (13, 1) for k in hs.PER_CHAIN}
        shapes.update({"stats_len_attempts.npy": (1, 3), "stats_len_accepts.npy": (1, 3), "stats_site_changes.npy": (1, L)})
        args = drv.build_parser().parse_args(common + ["--results_path", res, "--run_signature", "stats", "--ppde_stats"])
        args.ppde_reuse_grad = True
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = drv.main(args)
        assert len(re.findall(line, buf.getvalue())) == 1
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))} == old | set(shapes)
        for f, shape in shapes.items():
            a = np.load(os.path.join(out, f))
            assert a.shape == shape and a.dtype == np.int64, f
        assert (np.load(os.path.join(out, "stats_iters.npy")) == 40).all()
        args = drv.build_parser().parse_args(common + ["--results_path", res, "--run_signature", "nosites", "--ppde_stats_no_sites"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out_ns = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out_ns, "*"))} == old | (set(shapes) - {"stats_site_changes.npy"})
        args = drv.build_parser().parse_args(common + ["--results_path", res, "--run_signature", "plain"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out_plain = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out_plain, "*"))} == old    # off by default: nothing new
        # two gloo ranks on one card, as fresh child processes: chains split 7 + 6, every file equal to the single-rank one
        env = dict(os.environ, PPDE_ONE_GPU="1", PPDE_DIST_BACKEND="gloo", OMP_NUM_THREADS="2")
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                            "127.0.0.1", "--master-port", "29547", script, *common, "--results_path", res2, "--run_signature", "stats",
                            "--ppde_stats", "--ppde_shard"], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        out2 = glob.glob(os.path.join(res2, "TOY24", "*"))[0]
        for f in list(shapes) + ["energy_history.npy", "population.npy"]:
            assert np.array_equal(np.load(os.path.join(out, f)), np.load(os.path.join(out2, f))), f
        # every rank logs the whole population's figures (the two ranks share one pipe: a line may be cut by the other rank's)
        assert set(re.findall(line, r.stdout)) == set(re.findall(line, buf.getvalue()))

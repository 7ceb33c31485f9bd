"""The archive on the GPU (ppde_chains_set_archive; k_archive in ppde_amd/csrc/archive.h): what it holds equals the online rule
(helpers_archive.archive_of, the only reference) applied to the peeks of a twin run -- the same run without an archive, stepped
one iteration at a time -- in idx, energy bits, fitness bits, step and count: in every mode, under both gradient policies, from
graphs and eagerly, on caller-supplied noise, at every layout edge of the state row; and the archiving run's results are the
twin's. Everything is exact (array_equal, floats compared as bits).

Each test asserts on its twin that the branch it means to check was taken (helpers_archive.events): evictions, duplicates at an
iteration where the state changed, refusals at equal energy, wild-type skips, chains that end below K.
tests/test_archive_cpu.py asserts the same conditions on CPU reference runs of the toy configurations. For the layout-edge
geometries (helpers_archive.edge_case, Philox seed 700 + n) the CPU reference of 5 chains shows, at L = 8 / 70 / 104 / 237 / 252 /
253 / 307, 158 / 114 / 67 / 91 / 50 / 66 / 86 refusals at equal energy and 17 / 15 / 10 / 9 / 11 / 20 / 7 changed duplicates (65
chains at L = 8 / 70 / 104: 2287 / 1528 / 878 and 170 / 162 / 126)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_archive as ha
import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
ARCHIVE_KEYS = ("idx", "energy", "fitness", "step", "count")
N, T_LONG, PAS, NMUT, SEED = 16, 130, 2, 3, 202           # 130 = one 100 segment, one 20 segment and 10 eager steps
BETAS = ht.REPLAY_BETAS
MODES = ("default", "library", "reversible", "tempering")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_archive_equal(got, want, label):
    assert got["idx"].dtype == np.uint8 and got["energy"].dtype == np.float32 and got["step"].dtype == np.int32
    for k in ARCHIVE_KEYS:
        assert got[k].shape == want[k].shape, (label, k)
    assert np.array_equal(got["count"], want["count"]), (label, "count", got["count"], want["count"])
    assert np.array_equal(got["step"], want["step"]), (label, "step")
    assert np.array_equal(got["idx"], want["idx"]), (label, "idx")
    assert np.array_equal(_bits(got["energy"]), _bits(want["energy"])), (label, "energy")
    assert np.array_equal(_bits(got["fitness"]), _bits(want["fitness"])), (label, "fitness")


def _make(m, c, lib, mode, n, T, rng_mode=1, reuse=True, swap_every=1, archive=None, x0=None, lo=None, hi=None, nmut=NMUT,
          betas=BETAS, which=None, before=None, after=None, **kw):
    """`before` / `after`: callables that set a recorder / pair counts on the chains before / after the archive is set."""
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", SEED)
    lo = c["i0"] if lo is None else lo
    hi = c["i0"] + c["Lp"] - 1 if hi is None else hi
    which = (3 if c.get("cnn") is not None else 1) if which is None else which
    ch = Chains(m, n, T, PAS, nmut, False, lo, hi, which, rng_mode, reuse_grad=reuse, **kw)
    if mode != "default":
        ch.set_library(lib)
    if mode in ("reversible", "tempering"):
        ch.set_reversible(True)
    if mode == "tempering":
        ch.set_tempering(betas, swap_every)
    if before is not None:
        before(ch)
    if archive is not None:
        ch.set_archive(archive)
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


@pytest.fixture(scope="module")
def law():
    c = dict(hl.law_case(), cnn=None, lamda=0.0)
    m = hl.hip_model_of(c)
    yield c, c["allowed"], m
    m.close()


_TWINS = {}


def _noise(c, T):
    import ppde_oracle as orc
    gen = torch.Generator().manual_seed(77)
    return [orc.draw_noise_torch(N, c["L"] * 20, PAS, generator=gen) for _ in range(T)]


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


def _twin(name, case, mode, reuse, rng_mode=1, T=T_LONG, **kw):
    """The run WITHOUT an archive, stepped one iteration at a time and peeked after each: computed once per configuration."""
    key = (name, mode, reuse, rng_mode, T, tuple(sorted(kw.items())))
    if key not in _TWINS:
        c, lib, m = case
        ch = _make(m, c, lib, mode, N, T, rng_mode, reuse, trace=True, **kw)
        peeks = _stepped(ch, T, _noise(c, T) if rng_mode == 0 else None)
        _TWINS[key] = dict(peeks=peeks, res=ch.collect(), tr=ch.trace(), hist=ch.tempering_history() if mode == "tempering" else None)
        ch.close()
    return _TWINS[key]


def _archiving_run(case, mode, reuse, K, rng_mode=1, T=T_LONG, **kw):
    c, lib, m = case
    ch = _make(m, c, lib, mode, N, T, rng_mode, reuse, archive=K, trace=True, **kw)
    if rng_mode == 0:
        _feed(ch, _noise(c, T))
    else:
        ch.run(T)
        gs = ch.graph_stats()
        assert (gs["replayed_steps"], gs["eager_steps"]) == ((T // 20) * 20, T % 20)           # graphs and eager issue both ran
        assert gs["captures_in_run"] == 0
    out = dict(arc=ch.archive(), res=ch.collect(), tr=ch.trace(), hist=ch.tempering_history() if mode == "tempering" else None)
    ch.close()
    return out


def _assert_nothing_else_changed(out, twin, label):
    for k in RESULT_KEYS:
        assert np.array_equal(out["res"][k], twin["res"][k]), (label, k)
    for k in TRACE_KEYS:
        assert np.array_equal(out["tr"][k], twin["tr"][k]), (label, k)
    if twin["hist"] is not None:
        assert np.array_equal(out["hist"], twin["hist"]), label


def _resets(twin, wt):
    """Mutation-cap resets of a default-mode twin: iterations after which the peeked state is not the state the trace leads to."""
    tr, prev, resets = twin["tr"], twin["peeks"][0]["idx"].copy(), 0
    for t in range(tr["accepted"].shape[0]):
        pre = prev.copy()
        for b in np.flatnonzero(tr["accepted"][t]):
            for s in range(int(tr["U"][t, b])):
                l, k = divmod(int(tr["flat"][t, s, b]), 20)
                pre[b, l] = k
        now = twin["peeks"][t + 1]["idx"]
        differs = (pre != now).any(1)
        assert (now[differs] == wt[None]).all()                                                  # a reset goes to the wild type
        resets += int(differs.sum())
        prev = now
    return resets


# ------------------------------------------------------------------------------------------------ 1. the rule, toy sizes
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_the_archive_is_the_online_rule_on_the_twins_peeks(toy, mode, reuse):
    """TOY24, 16 chains, pas_length 2, nmut_threshold 3, T = 130 on the device RNG, K = 1, 3, 32; the results are the twin's."""
    c, _, _ = toy
    twin = _twin("toy", toy, mode, reuse)
    assert twin["tr"]["accepted"].any() and not twin["tr"]["accepted"].all()
    if mode == "default":
        resets = _resets(twin, c["wt"])
        assert resets >= 1, "no mutation-cap reset in this run: the skipped pair is not exercised"
    for K in (1, 3, 32):
        label = f"{mode} reuse={reuse} K={K}"
        ev = ha.events(twin["peeks"], K)
        print(label, ev)
        assert ev["insertions"] >= N and ev["duplicates"] >= 1, (label, ev)
        assert ev["evictions"] >= 1 or (K == 32 and mode != "reversible"), (label, ev)
        if mode == "reversible":
            assert ev["changed_duplicates"] >= 1, (label, ev)
        if mode == "default":
            assert ev["wt_skips"] >= resets, (label, ev)
            if K == 32:
                assert ev["short_chains"] >= 1, (label, ev)
        out = _archiving_run(toy, mode, reuse, K)
        _assert_archive_equal(out["arc"], ha.archive_of(twin["peeks"], K), label)
        _assert_nothing_else_changed(out, twin, label)


def test_the_archive_is_the_online_rule_on_caller_supplied_noise(toy):
    """rng_mode 0 (every iteration its own eager launch sequence), T = 12, default and reversible."""
    T = 12
    for mode in ("default", "reversible"):
        twin = _twin("toy", toy, mode, True, rng_mode=0, T=T)
        for K in (1, 3, 32):
            ev = ha.events(twin["peeks"], K)
            assert ev["insertions"] >= 1, (mode, K, ev)
            out = _archiving_run(toy, mode, True, K, rng_mode=0, T=T)
            _assert_archive_equal(out["arc"], ha.archive_of(twin["peeks"], K), f"{mode} rng_mode 0 K={K}")
            _assert_nothing_else_changed(out, twin, f"{mode} rng_mode 0 K={K}")
        assert ha.events(twin["peeks"], 1)["evictions"] >= 1, mode


@pytest.mark.parametrize("mode", ["reversible", "tempering"])
def test_the_archive_on_a_small_state_space_where_chains_come_back(law, mode):
    """helpers_library.law_case (35 states), 16 chains, T = 130, no cap, K = 1, 4, 16, 32: most candidates are states the chain has
    archived before, met again after a move."""
    c, _, _ = law
    kw = dict(lo=0, hi=c["L"] - 1, nmut=0)
    twin = _twin("law", law, mode, True, **kw)
    for K in (1, 4, 16, 32):
        label = f"law_case {mode} K={K}"
        ev = ha.events(twin["peeks"], K)
        print(label, ev)
        assert ev["changed_duplicates"] >= 1, (label, ev)
        if mode == "reversible":
            assert ev["evictions"] >= 1 or K == 32, (label, ev)
            if K == 32:
                assert ev["short_chains"] == N, (label, ev)                                     # 34 archivable states: never full
        out = _archiving_run(law, mode, True, K, **kw)
        _assert_archive_equal(out["arc"], ha.archive_of(twin["peeks"], K), label)
        _assert_nothing_else_changed(out, twin, label)


# ------------------------------------------------------------------------------------------------ 2. layout edges
@pytest.mark.parametrize("L", ha.EDGE_LENGTHS)
def test_the_archive_at_the_layout_edges(L):
    """helpers_archive.edge_case: state rows of 5 to 79 dwords (one or two per lane; the last dword of the row partly or wholly
    pad), open residues at both ends of the row and astride a dword boundary, energies shared by the states that differ only
    outside the Potts window; populations on both sides of a workgroup's four chains; reversible mode over the full range, K = 4,
    T = 60."""
    c, lib, sites = ha.edge_case(L)
    m = hl.hip_model_of(c)
    K, T = ha.EDGE_K, ha.EDGE_T
    equal = changed = 0
    for n in ha.EDGE_POPULATIONS:
        kw = dict(lo=0, hi=L - 1, nmut=0, seed=700 + n, random_chain=-1)
        ch = _make(m, c, lib, "reversible", n, T, **kw)
        peeks = _stepped(ch, T)
        res = ch.collect()
        ch.close()
        ev = ha.events(peeks, K)
        equal, changed = equal + ev["equal_refusals"], changed + ev["changed_duplicates"]
        ch = _make(m, c, lib, "reversible", n, T, archive=K, **kw)
        ch.run(T)
        arc, res_a = ch.archive(), ch.collect()
        ch.close()
        _assert_archive_equal(arc, ha.archive_of(peeks, K), f"L={L} n={n}")
        for k in RESULT_KEYS[:-1]:
            assert np.array_equal(res_a[k], res[k]), (L, n, k)
        live = np.arange(K)[None] < arc["count"][:, None]
        frozen = np.setdiff1d(np.arange(L), sites)
        assert (arc["idx"][live][:, frozen] == c["wt"][frozen][None]).all()
    m.close()
    print(f"L={L}: {equal} refusals at equal energy, {changed} changed duplicates")
    assert equal >= 1 and changed >= 1


# ------------------------------------------------------------------------------------------------ 3. all energies equal
def test_with_all_energies_equal_the_archive_is_the_first_k_distinct_states():
    c, lib, sites = ha.edge_case(70)
    c = dict(c, J=np.zeros_like(c["J"]), h=np.zeros_like(c["h"]))
    m = hl.hip_model_of(c)
    n, T, K = 5, 60, 4
    kw = dict(lo=0, hi=c["L"] - 1, nmut=0, seed=31, random_chain=-1)
    ch = _make(m, c, lib, "reversible", n, T, **kw)
    peeks = _stepped(ch, T)
    ch.close()
    ch = _make(m, c, lib, "reversible", n, T, archive=K, **kw)
    ch.run(T)
    arc = ch.archive()
    ch.close()
    m.close()
    ev = ha.events(peeks, K)
    assert ev["evictions"] == 0 and ev["equal_refusals"] >= 1 and ev["lower_refusals"] == 0, ev
    _assert_archive_equal(arc, ha.archive_of(peeks, K), "all energies equal")
    for b in range(n):                                                                          # the first K distinct, in visiting order
        seen, steps = [], []
        for t, pk in enumerate(peeks):
            key = pk["idx"][b].tobytes()
            if pk["dist"][b] and key not in seen and len(seen) < K:
                seen.append(key)
                steps.append(t)
        assert [r.tobytes() for r in arc["idx"][b, :arc["count"][b]]] == seen and arc["step"][b, :len(steps)].tolist() == steps
        assert len(np.unique(_bits(arc["energy"][b, :arc["count"][b]]))) == 1


# ------------------------------------------------------------------------------------------------ 4. next to recorder and pairs
@pytest.mark.parametrize("mode", MODES)
def test_recorder_and_pair_counts_next_to_the_archive_hold_what_they_held(toy, mode):
    c, lib, m = toy
    T, K = 40, 3

    def rec_and_pairs(ch):
        ch.set_recorder(every=3, burn_in=2)
        ch.set_pair_counts(None)

    def run(**kw):
        ch = _make(m, c, lib, mode, N, T, **kw)
        ch.run(T)
        rec = "before" in kw or "after" in kw
        out = dict(rec=ch.recorded() if rec else None, pairs=ch.pair_counts() if rec else None,
                   arc=ch.archive() if kw.get("archive") else None, res=ch.collect())
        ch.close()
        return out

    plain = run(before=rec_and_pairs)
    only = run(archive=K)
    for order in ("before", "after"):
        both = run(archive=K, **{order: rec_and_pairs})
        for k in ("idx", "energy", "fitness", "chain", "site_counts"):
            assert np.array_equal(both["rec"][k], plain["rec"][k]), (mode, order, k)
        assert both["rec"]["rows"] == plain["rec"]["rows"] == (T - 2) // 3
        assert np.array_equal(both["pairs"][0], plain["pairs"][0]) and np.array_equal(both["pairs"][1], plain["pairs"][1])
        _assert_archive_equal(both["arc"], only["arc"], f"{mode} {order}")
        for k in RESULT_KEYS:
            assert np.array_equal(both["res"][k], plain["res"][k]), (mode, order, k)


# ------------------------------------------------------------------------------------------------ 5. the running best
def test_entry_zero_is_the_running_best_in_reversible_mode(toy):
    c, _, _ = toy
    checked = 0
    for K in (1, 3, 32):
        out = _archiving_run(toy, "reversible", True, K)
        arc, res = out["arc"], out["res"]
        for b in np.flatnonzero((res["best_idx"] != c["wt"][None]).any(1)):
            assert arc["count"][b] >= 1
            assert np.array_equal(arc["idx"][b, 0], res["best_idx"][b]), (K, b)
            assert _bits(arc["energy"][b, 0]) == _bits(res["best_energy"][b]) and _bits(arc["fitness"][b, 0]) == _bits(res["best_fitness"][b])
            assert arc["step"][b, 0] == res["best_step"][b], (K, b)
            checked += 1
    assert checked >= 3 * N // 2


# ------------------------------------------------------------------------------------------------ 6. the default mode's cap
def test_under_a_cap_every_entry_is_a_state_the_chain_continued_from_with_its_own_energy(toy):
    c, _, m = toy
    for reuse in (True, False):
        out = _archiving_run(toy, "default", reuse, 32)
        arc = out["arc"]
        live = np.arange(32)[None] < arc["count"][:, None]
        states = arc["idx"][live]
        d = (states != c["wt"][None]).sum(1)
        assert states.shape[0] >= N and ((d >= 1) & (d < NMUT)).all()
        e, fit, _ = m.energy_grad(torch.from_numpy(np.ascontiguousarray(states)), 3, False)
        assert np.array_equal(_bits(e.cpu().numpy()), _bits(arc["energy"][live])), reuse
        assert np.array_equal(_bits(fit.cpu().numpy()), _bits(arc["fitness"][live])), reuse
        # the running best may sit AT the cap, where the archive never goes
        at_cap = ((out["res"]["best_idx"] != c["wt"][None]).sum(1) >= NMUT)
        print(f"reuse={reuse}: {int(at_cap.sum())} chains whose best state is at the cap")


# ------------------------------------------------------------------------------------------------ 7. interfaces
def test_archive_refusals_first_row_second_init_and_clearing(toy):
    from ppde_amd import _hip
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    n, T, L = 8, 40, c["L"]
    bad = pytest.raises
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no archive was set"):
        ch.archive()
    assert ch.lib.ppde_chains_archive_read(ch.handle, None, None, None, None, None) == -1
    for k in (0, -1, 33, 1000):
        with bad(_hip.PpdeHipError, match=r"\[-1\].*k must be in 1\.\.32"):
            ch.set_archive(k)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no archive was set"):                          # every refusal left the object unchanged
        ch.archive()
    ch.set_archive(32)
    ch.set_archive(None)                                                                      # cleared
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no archive was set"):
        ch.archive()
    ch.set_archive(2)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*not initialised"):
        ch.archive()
    # a start away from the wild type: the read before any run holds row 0 only
    x0 = np.tile(c["wt"], (n, 1))
    for b in range(1, n):
        x0[b, lo + b] = (x0[b, lo + b] + 1) % 20
    ch.init(torch.as_tensor(x0).cuda())
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_archive(4)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_archive(None)
    first, pk = ch.archive(), ch.peek()
    _assert_archive_equal(first, ha.archive_of([pk], 2), "row 0")
    assert first["count"].tolist() == [0] + [1] * (n - 1) and (first["step"][1:, 0] == 0).all() and (first["idx"][0] == 255).all()
    assert np.array_equal(first["idx"][1:, 0], x0[1:]) and np.isneginf(first["energy"][:, 1]).all()
    ch.run(30)
    later = ch.archive()
    assert (later["count"] >= first["count"]).all() and later["count"].sum() > first["count"].sum()
    assert ch.lib.ppde_chains_archive_read(ch.handle, None, None, None, None, None) == 0       # any pointer may be NULL
    k = ctypes.c_int32()
    _hip.check(ch.lib.ppde_chains_archive_shape(ch.handle, ctypes.byref(k)))
    assert k.value == 2 and ch.lib.ppde_chains_archive_shape(ch.handle, None) == 0
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())                                 # a second init empties it
    again = ch.archive()
    assert (again["count"] == 0).all() and (again["idx"] == 255).all() and (again["step"] == -1).all()
    ch.run(30)
    twin = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    twin.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    peeks = [twin.peek()]
    for _ in range(30):
        twin.run(1)
        peeks.append(twin.peek())
    twin.close()
    _assert_archive_equal(ch.archive(), ha.archive_of(peeks, 2), "after a second init")
    ch.close()
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7, n_streams=2)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*n_streams > 1"):
        ch.set_archive(4)
    ch.close()
    ch = Chains(m, n, T, 2, 3, True, lo, hi, 3, 1, seed=7)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*paper_results"):
        ch.set_archive(4)
    ch.close()


def test_sharding_does_not_change_the_archives_or_the_candidates(toy):
    from ppde_amd.archive import merge
    c, lib, m = toy
    T, K = 45, 3

    def run(mode, n_, off):
        ch = _make(m, c, lib, mode, n_, T, archive=K, chain_offset=off, random_chain=-1, seed=99)
        ch.run(T)
        a = ch.archive()
        ch.close()
        return a

    for mode in MODES:
        one, a, b = run(mode, 16, 0), run(mode, 8, 0), run(mode, 8, 8)
        joined = {k: np.concatenate([a[k], b[k]], 0) for k in ARCHIVE_KEYS}
        _assert_archive_equal(joined, one, mode)
        whole, parts = merge(*[one[k] for k in ARCHIVE_KEYS]), merge(*[joined[k] for k in ARCHIVE_KEYS])
        assert whole["idx"].shape[0] >= 1 and (whole["n_chains"] >= 1).all()
        for k in whole:
            assert np.array_equal(whole[k], parts[k]), (mode, k)
        assert (np.diff(whole["energy"]) <= 0).all() and len({r.tobytes() for r in whole["idx"]}) == whole["idx"].shape[0]
        # a shard merged on its own carries its global chains
        assert set(merge(*[b[k] for k in ARCHIVE_KEYS], chain_offset=8)["chain"].tolist()) <= set(range(8, 16))


def test_ppde_pas_and_the_driver_hand_the_archive_out():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd import synthetic
    from ppde_amd.archive import merge
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    L = len(seq)
    n, T, pas, nmut, seed, K = 8, 30, 2, 3, 4242, 4
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        base = dict(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n, device="cuda:0",
                    ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox", ppde_seed=seed)
        en = ProteinProductOfExperts(argparse.Namespace(**base))
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        runs = []
        for k in (None, K):
            np.random.seed(5)
            with contextlib.redirect_stdout(io.StringIO()):
                sampler = PPDE_PAS(argparse.Namespace(**base, ppde_archive=k))
                runs.append(sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10))
            if k is None:
                assert sampler.archive is None
        assert len(runs[1]) == 6                                                             # the returned tuple does not change
        assert torch.equal(runs[0][0], runs[1][0])
        for k in range(1, 5):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        assert all(np.array_equal(a, b) for a, b in zip(runs[0][5], runs[1][5]))
        np.random.seed(5)
        ch = Chains(en.model, n, T, pas, nmut, False, i0, i0 + Lp - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_archive(K)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        want = ch.archive()
        ch.close()
        got = sampler.archive
        _assert_archive_equal({k: got[k] for k in ARCHIVE_KEYS}, want, "PPDE_PAS")
        assert np.array_equal(got["chain"], np.arange(n)) and got["count"].sum() >= n
        cand = merge(*[want[k] for k in ARCHIVE_KEYS])
        assert set(got["candidates"]) == {"idx", "energy", "fitness", "chain", "step", "n_chains"}
        for k in cand:
            assert np.array_equal(got["candidates"][k], cand[k]), k
        # the driver: the listed files with these shapes, beside the existing ones
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_archive", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        common = ["--protein_weights", root, "--protein", "TOY24", "--results_path", res, "--device", "cuda:0",
                  "--disable_MSA_transformer_scoring", "--n_chains", "12", "--n_iters", "40", "--seed", "3", "--log_every", "25",
                  "--nmut_threshold", "4", "--ppde_rng", "philox"]
        old = {"config.txt", "population.npy", "pred_fitness_scores.npy", "oracle_fitness_scores.npy", "potts_scores.npy",
               "energy_scores.npy", "energy_history.npy", "fitness_history.npy"}
        per_chain = {"archive.npy": (12, 5, L), "archive_energy.npy": (12, 5), "archive_fitness.npy": (12, 5), "archive_step.npy": (12, 5),
                     "archive_count.npy": (12,)}
        merged = ("candidates.npy", "candidates_energy.npy", "candidates_fitness.npy", "candidates_chain.npy", "candidates_step.npy",
                  "candidates_nchains.npy")
        args = drv.build_parser().parse_args(common + ["--run_signature", "archive", "--ppde_archive", "5"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))} == old | set(per_chain) | set(merged)
        for f, shape in per_chain.items():
            assert np.load(os.path.join(out, f)).shape == shape, f
        M = np.load(os.path.join(out, "candidates.npy")).shape[0]
        assert M >= 1 and np.load(os.path.join(out, "candidates.npy")).shape == (M, L)
        for f in merged[1:]:
            assert np.load(os.path.join(out, f)).shape == (M,), f
        ar, cnt = np.load(os.path.join(out, "archive.npy")), np.load(os.path.join(out, "archive_count.npy"))
        assert ar.dtype == np.uint8 and cnt.sum() >= M and (np.diff(np.load(os.path.join(out, "candidates_energy.npy"))) <= 0).all()
        args = drv.build_parser().parse_args(common + ["--run_signature", "plain"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(args)
        assert {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))} == old          # off by default: nothing new


def test_the_archive_on_the_eager_path_of_a_transformer_run():
    """Potts + CNN + a two-layer transformer expert (tests/test_modes_gpu.py's toy geometry): such runs are never captured, every
    iteration is issued eagerly. T = 6, 4 chains, reversible mode, K = 3, against its own twin."""
    import helpers_modes as hm
    from ppde_amd.energy import HipModel
    wt, J, h, cnn, st = hm.toy_parts()
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, hm.TOY["win"][0])
    m.set_cnn(cnn)
    m.set_transformer(st, hm.TOY["heads"])
    m.set_lamda(hm.LAMDA)
    c = dict(wt=wt, L=hm.TOY["L"], i0=hm.TOY["win"][0], Lp=hm.TOY["win"][1], cnn=cnn)
    lib = hm.window_library(wt, hm.TOY["win"])
    n, T, K = 4, 6, 3
    kw = dict(lo=0, hi=c["L"] - 1, nmut=0, which=7, seed=11, random_chain=-1)
    ch = _make(m, c, lib, "reversible", n, T, **kw)
    peeks = _stepped(ch, T)
    res = ch.collect()
    ch.close()
    ch = _make(m, c, lib, "reversible", n, T, archive=K, **kw)
    ch.run(T)
    gs = ch.graph_stats()
    assert (gs["captures"], gs["replayed_steps"], gs["eager_steps"]) == (0, 0, T)
    arc, res_a = ch.archive(), ch.collect()
    ch.close()
    m.close()
    assert ha.events(peeks, K)["insertions"] >= 1
    _assert_archive_equal(arc, ha.archive_of(peeks, K), "transformer")
    for k in RESULT_KEYS[:-1]:
        assert np.array_equal(res_a[k], res[k]), k

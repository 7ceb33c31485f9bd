"""The archive without a GPU: the online rule on hand-made histories, its agreement with the offline "K best distinct states" when
energy is a function of the state, ppde_amd.archive.merge, what PPDE_PAS refuses before any device work, the driver's flag, the
host side of the C ABI as a stand-alone program under AddressSanitizer (tests/hostcheck/archive.cpp), and the conditions the GPU
tests of tests/test_archive_gpu.py stand on, asserted on CPU reference runs of the same configurations.

Measured on those references (16 chains, T = 130, pas_length 2, Philox seed 202, helpers_archive.events):
  TOY24, reversible, nmut 3: evictions 73 / 136 / 154 and changed duplicates 2 / 4 / 11 at K = 1 / 3 / 32;
  TOY24, default mode, nmut 3: 298 resets, 601 wild-type skips, evictions 41 / 101 / 4 at K = 1 / 3 / 32, 15 chains below K = 32;
  law_case, reversible, nmut 0: evictions 39 / 75 / 61 / 0 and changed duplicates 193 / 544 / 1007 / 1030 at K = 1 / 4 / 16 / 32,
    no chain fills K = 32.
The tests assert ">= 1" of each kind, not these counts."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_archive as ha
import helpers_library as hl
import helpers_reversible as hr

WT = np.array([0, 0, 0, 0], np.uint8)
A_, B_, C_, D_, E_ = ([1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 3, 0], [0, 0, 0, 4], [5, 5, 0, 0])


def _arch(rows, K):
    return ha.archive_of(ha.hand_peeks(rows, WT), K)


def _states(a, b=0):
    return [tuple(r) for r in a["idx"][b, :a["count"][b]]]


# ------------------------------------------------------------------------------------------------ the rule
def test_ties_are_evicted_by_the_latest_step():
    a = _arch([(WT, 9.0), (A_, 1.0), (B_, 1.0), (C_, 1.0), (D_, 2.0)], 3)                       # A, B, C tie at 1: C (step 3) goes
    assert _states(a) == [tuple(D_), tuple(A_), tuple(B_)]
    assert a["step"][0].tolist() == [4, 1, 2] and a["energy"][0].tolist() == [2.0, 1.0, 1.0]
    a = _arch([(A_, 1.0), (B_, 1.0), (C_, 1.0), (D_, 2.0), (E_, 3.0)], 3)                       # then B (step 1)
    assert _states(a) == [tuple(E_), tuple(D_), tuple(A_)] and a["step"][0].tolist() == [4, 3, 0]
    assert ha.events(ha.hand_peeks([(A_, 1.0), (B_, 1.0), (C_, 1.0), (D_, 2.0), (E_, 3.0)], WT), 3)["evictions"] == 2


def test_the_comparison_is_strict_at_equal_energy():
    rows = [(A_, 1.0), (B_, 2.0), (C_, 1.0), (D_, 0.5)]
    a = _arch(rows, 2)
    assert _states(a) == [tuple(B_), tuple(A_)] and a["step"][0].tolist() == [1, 0]
    ev = ha.events(ha.hand_peeks(rows, WT), 2)
    assert (ev["equal_refusals"], ev["lower_refusals"], ev["evictions"]) == (1, 1, 0)
    assert _arch([(A_, 0.0), (B_, -0.0)], 1)["step"][0].tolist() == [0]                         # -0 == +0: no eviction
    a = _arch([(A_, 1.0), (A_, 5.0), (A_, 0.5)], 2)                                             # a duplicate keeps its first energy and step
    assert a["count"][0] == 1 and a["energy"][0, 0] == 1.0 and a["step"][0, 0] == 0


def test_a_state_that_was_evicted_re_enters_with_its_later_step():
    a = _arch([(A_, 1.0), (B_, 2.0), (C_, 3.0), (A_, 4.0)], 2)                                  # A out at step 2, back at step 3
    assert _states(a) == [tuple(A_), tuple(C_)] and a["step"][0].tolist() == [3, 2] and a["energy"][0].tolist() == [4.0, 3.0]
    ev = ha.events(ha.hand_peeks([(A_, 1.0), (B_, 2.0), (C_, 3.0), (A_, 4.0)], WT), 2)
    assert ev["evictions"] == 2 and ev["duplicates"] == 0


def test_energies_that_are_not_finite_are_skipped_and_the_wild_type_is_never_present():
    rows = [(WT, 50.0), (A_, float("nan")), (B_, float("inf")), (C_, float("-inf")), (D_, -3.0), (WT, 99.0), (A_, 1.0)]
    a = _arch(rows, 4)
    assert _states(a) == [tuple(A_), tuple(D_)] and a["step"][0, :2].tolist() == [6, 4] and a["count"][0] == 2
    ev = ha.events(ha.hand_peeks(rows, WT), 4)
    assert (ev["wt_skips"], ev["nonfinite_skips"], ev["insertions"], ev["short_chains"]) == (2, 3, 2, 1)
    assert (a["idx"][0, 2:] == 255).all() and np.isneginf(a["energy"][0, 2:]).all()
    assert (a["fitness"][0, 2:] == 0).all() and (a["step"][0, 2:] == -1).all()
    assert not any((r == WT).all() for r in a["idx"][0, :2])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_online_rule_keeps_the_k_best_distinct_states(seed):
    """Seeded random histories over a small state space in which energy is a function of the state and distinct states have
    distinct energies: the online archive holds exactly the offline top K, for every K."""
    rng = np.random.default_rng(seed)
    S, T, n, L = 40, 300, 6, 5
    states = np.unique(rng.integers(0, 3, (S, L)).astype(np.uint8), axis=0)
    energy = rng.permutation(states.shape[0]).astype(np.float32) - 7.0                          # distinct
    wt = states[0]
    visits = rng.integers(0, states.shape[0], (T + 1, n))
    hist = states[visits]
    peeks = ha.peeks_of(hist, energy[visits], -energy[visits], wt)
    assert sum(int((p["dist"] == 0).sum()) for p in peeks) > 0
    for K in (1, 2, 7, 32):
        a = ha.archive_of(peeks, K)
        for b in range(n):
            got = {r.tobytes() for r in a["idx"][b, :a["count"][b]]}
            assert got == ha.top_distinct(hist[:, b], energy[visits[:, b]], [p["dist"][b] for p in peeks], K), (K, b)
            assert (np.diff(a["energy"][b, :a["count"][b]]) < 0).all()                           # sorted, energy descending
    assert ha.events(peeks, 2)["evictions"] > 0 and ha.events(peeks, 2)["changed_duplicates"] > 0


# ------------------------------------------------------------------------------------------------ merge
def test_merge_on_hand_made_archives():
    from ppde_amd.archive import merge
    K, L = 3, 4
    idx = np.full((4, K, L), 255, np.uint8)
    e = np.full((4, K), -np.inf, np.float32)
    f = np.zeros((4, K), np.float32)
    s = np.full((4, K), -1, np.int32)
    count = np.array([3, 2, 0, 1], np.int32)

    def put(b, j, st, en, step):
        idx[b, j], e[b, j], f[b, j], s[b, j] = st, en, 10.0 * b + j, step

    put(0, 0, A_, 5.0, 7); put(0, 1, B_, 4.0, 2); put(0, 2, C_, 1.0, 9)
    put(1, 0, B_, 6.0, 3); put(1, 1, A_, 5.0, 1)                                                # A at the same energy: chain 0 is kept
    put(3, 0, C_, 1.0, 4)                                                                       # chain 2 is empty
    m = merge(idx, e, f, s, count, chain_offset=100)
    assert [tuple(r) for r in m["idx"]] == [tuple(B_), tuple(A_), tuple(C_)]
    assert m["energy"].tolist() == [6.0, 5.0, 1.0] and m["chain"].tolist() == [101, 100, 100]
    assert m["step"].tolist() == [3, 7, 9] and m["n_chains"].tolist() == [2, 2, 2] and m["fitness"].tolist() == [10.0, 0.0, 2.0]
    assert m["idx"].dtype == np.uint8 and m["chain"].dtype == np.int64 and m["n_chains"].dtype == np.int32
    # order among equal energies: chain ascending, then step
    put(3, 0, D_, 5.0, 0)
    m = merge(idx, e, f, s, count)
    assert [tuple(r) for r in m["idx"]] == [tuple(B_), tuple(A_), tuple(D_), tuple(C_)] and m["chain"].tolist() == [1, 0, 3, 0]
    assert m["n_chains"].tolist() == [2, 2, 1, 1]
    empty = merge(idx, e, f, s, np.zeros(4, np.int32))
    assert empty["idx"].shape == (0, L) and empty["energy"].shape == (0,) and empty["n_chains"].shape == (0,)
    with pytest.raises(ValueError, match="count"):
        merge(idx, e, f, s, np.array([4, 0, 0, 0]))
    # merging the halves of a population with their offsets is merging the whole
    whole = merge(idx, e, f, s, count)
    a, b = merge(idx[:2], e[:2], f[:2], s[:2], count[:2]), merge(idx[2:], e[2:], f[2:], s[2:], count[2:], chain_offset=2)
    assert set(map(bytes, whole["idx"])) == set(map(bytes, a["idx"])) | set(map(bytes, b["idx"]))


# ------------------------------------------------------------------------------------------------ PPDE_PAS, the driver
class _NoDevice:
    which = 1

    def __getattr__(self, name):
        raise AssertionError(f"PPDE_PAS touched the model ({name}) before refusing")


def _args(**kw):
    base = dict(ppde_pas_length=2, nmut_threshold=0, paper_results=False, ppde_rng="philox", seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_ppde_pas_archive_spellings_and_refusals_come_before_any_device_work():
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(_args()).archive_k == 0 and PPDE_PAS(_args()).archive is None                # off by default
    for off in (None, 0):
        assert PPDE_PAS(_args(ppde_archive=off)).archive_k == 0
    for k in (1, 8, 32):
        assert PPDE_PAS(_args(ppde_archive=k)).archive_k == k
    for bad in (-1, 33, 100, 2.5, "many", True):
        with pytest.raises(ValueError, match="ppde_archive.*1..32"):
            PPDE_PAS(_args(ppde_archive=bad))
    with pytest.raises(ValueError, match="ppde_archive.*paper_results"):
        PPDE_PAS(_args(ppde_archive=4, paper_results=True))
    assert PPDE_PAS(_args(paper_results=True)).archive_k == 0                                   # ... which alone stays what it was
    with pytest.raises(ValueError, match="ppde_archive.*ppde_streams"):
        PPDE_PAS(_args(ppde_archive=4, ppde_streams=2))
    # a valid K goes on to the device (here: to the stand-in, which says so)
    from ppde_amd.encoding import idx_to_onehot
    c = hl.law_case()
    x0 = torch.from_numpy(idx_to_onehot(np.tile(c["wt"], (4, 1)))).float()
    with pytest.raises(AssertionError, match="touched the model"):
        PPDE_PAS(_args(ppde_archive=4)).run(x0, 5, argparse.Namespace(model=_NoDevice(), which=1), 0, c["L"] - 1, None)


def test_cli_flag_parses_into_the_sampler_argument():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli_archive", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build_parser().parse_args(["--ppde_archive", "8"]).ppde_archive == 8
    d = mod.build_parser().parse_args([])
    assert d.ppde_archive == 0
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(argparse.Namespace(**{**vars(d), "ppde_library": None})).archive_k == 0      # the defaults switch nothing on
    assert PPDE_PAS(argparse.Namespace(**{**vars(mod.build_parser().parse_args(["--ppde_archive", "8"])), "ppde_library": None})).archive_k == 8


# ------------------------------------------------------------------------------------------------ the host layer
def test_host_layer_of_the_archive_under_address_sanitizer():
    """tests/hostcheck/archive.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime of
    tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: every refusal, then set, shape, init, run, read, a second
    init, clear and destroy, then the walk once per fallible runtime call with that call failing. Any leak or out-of-bounds access
    fails the run."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "archive", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck archive ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ what the GPU tests stand on
N, T, PAS, SEED = 16, 130, 2, 202


def _reference_peeks(c, lib, mode, nmut, lo, hi):
    import ppde_oracle as orc
    en = hl.oracle_energy_of(c)
    x0 = np.tile(c["wt"].astype(np.int64), (N, 1))

    def noise(t):
        return orc.device_noise(SEED, 0, N, t, PAS, c["L"])

    if mode == "reversible":
        r = hr.reversible_run(en, x0, c["wt"], noise, T, lo, hi, PAS, nmut, allowed=lib)
    else:
        r = orc.run(en, x0, c["wt"], noise, T, lo, hi, PAS, nmut, record_after_reset=True)       # (states as peek shows them)
    return ha.peeks_of(r["states"].numpy(), r["energy_history"].numpy(), r["fitness_history"].numpy(), c["wt"]), r


def test_the_toy_configurations_evict_revisit_and_reset():
    c, lib = hr.replay_model()
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    peeks, _ = _reference_peeks(c, lib, "reversible", 3, lo, hi)
    for K in (1, 3, 32):
        ev = ha.events(peeks, K)
        print(f"TOY24 reversible nmut 3, K = {K}: {ev}")
        assert ev["evictions"] >= 1 and ev["changed_duplicates"] >= 1 and ev["insertions"] >= N * min(K, 2)
    peeks, r = _reference_peeks(c, lib, "default", 3, lo, hi)
    pre = ha.peeks_of(_pre_reset_states(c, lo, hi), r["energy_history"].numpy(), r["fitness_history"].numpy(), c["wt"])
    resets = sum(int(((a["idx"] != b["idx"]).any(1)).sum()) for a, b in zip(peeks, pre))
    print(f"TOY24 default nmut 3: {resets} resets")
    assert resets >= 1
    for K in (1, 3, 32):
        ev = ha.events(peeks, K)
        print(f"TOY24 default nmut 3, K = {K}: {ev}")
        assert ev["evictions"] >= 1 and ev["wt_skips"] >= resets
        a = ha.archive_of(peeks, K)
        d = (a["idx"] != c["wt"][None, None]).sum(2)
        live = np.arange(K)[None] < a["count"][:, None]
        assert ((d[live] >= 1) & (d[live] < 3)).all()                                           # only states the chain continued from
    assert ha.events(peeks, 32)["short_chains"] >= 1


def _pre_reset_states(c, lo, hi):
    import ppde_oracle as orc
    r = orc.run(hl.oracle_energy_of(c), np.tile(c["wt"].astype(np.int64), (N, 1)), c["wt"],
                lambda t: orc.device_noise(SEED, 0, N, t, PAS, c["L"]), T, lo, hi, PAS, 3, record_after_reset=False)
    return r["states"].numpy()


def test_the_law_case_revisits_states_at_every_k():
    c = hl.law_case()
    peeks, _ = _reference_peeks(c, c["allowed"], "reversible", 0, 0, c["L"] - 1)
    for K in (1, 4, 16, 32):
        ev = ha.events(peeks, K)
        print(f"law_case reversible, K = {K}: {ev}")
        assert ev["changed_duplicates"] >= 1
        assert ev["evictions"] >= 1 or K == 32
    assert ha.events(peeks, 32)["short_chains"] == N                                            # 35 states, 34 of them archivable: never full

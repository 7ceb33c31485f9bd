"""The mode fuzzer without a GPU (tests/helpers_fuzz_modes.py; the GPU side is tests/fuzz_modes.py under tests/test_fuzz_modes_gpu.py):
the seed lists the GPU module runs are a pure function of their seeds, discard at most one draw in eight, hold only configurations
the C ABI accepts, cover the axes the hand-picked mode tests leave alone, and the one comparison both sides call reports every fault
the reference runners know how to plant. The two lists with forbidden patterns (`patterns`, `patterns_graph_len_4`) are held to the
same and to their own list of what the vetoes of their reference runs must have fallen on; the three lists without are pinned line
by line to tests/golden/fuzz_modes_lists.txt, so that the pattern axis cannot move them."""
import os

import numpy as np
import pytest

import helpers_anneal_adaptive as haa
import helpers_fuzz_modes as fz
import helpers_motifs as hmot
from ppde_amd import motifs

PATTERN_LISTS = ("patterns", "patterns_graph_len_4")


def _kept(c, trials=None):
    return fz.kept(c["seed"], c["trials"] if trials is None else trials, c["dynamics"], c.get("graph_len", 0), c.get("forbid", False))


@pytest.fixture(scope="module")
def lists():
    return {name: _kept(c) for name, c in fz.GPU_CASES.items()}


@pytest.fixture(scope="module")
def pattern_configs(lists):
    return [pair for name in PATTERN_LISTS for pair in lists[name][0]]


@pytest.fixture(scope="module")
def configs(lists):
    return [pair for out, _ in lists.values() for pair in out]


def _same_patterns(a, b):
    return (a is None) == (b is None) and (a is None or (np.array_equal(a.elements, b.elements) and np.array_equal(a.lengths, b.lengths)))


def test_the_lists_without_patterns_are_the_ones_from_before_the_pattern_axis(lists):
    """draw(..., forbid=False) draws nothing new and consumes no variate: the describe() line of every kept configuration of the
    three lists, as written when the generator knew no patterns."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_modes_lists.txt")) as f:
        want = f.read().splitlines()
    got = [f"{name}: {fz.describe(cfg)}" for name in ("default_env", "graph_len_4", "general_kernels") for cfg, _ in lists[name][0]]
    assert len(want) == 24 + 24 + 8
    assert got == want
    assert [fz.GPU_CASES[k]["seed"] for k in ("default_env", "graph_len_4", "general_kernels")] == [43, 53, 33]
    assert not any("patterns" in cfg for name in ("default_env", "graph_len_4", "general_kernels") for cfg, _ in lists[name][0])


def _same_config(a, b):
    return _same_patterns(a.get("patterns"), b.get("patterns")) and a.get("allow_native") == b.get("allow_native") and \
        fz.describe(a) == fz.describe(b) and np.array_equal(a["start"], b["start"]) and np.array_equal(a["wt"], b["wt"]) and \
        (a["library"] is None) == (b["library"] is None) and (a["library"] is None or np.array_equal(a["library"], b["library"]))


def test_the_kept_lists_are_a_pure_function_of_the_seed(lists):
    """Drawn again from scratch (references and discards included), the first six kept configurations of every list are the same."""
    for name, c in fz.GPU_CASES.items():
        fz._KEPT.pop((c["seed"], 6, c["dynamics"], c.get("graph_len", 0)) + ((True,) if c.get("forbid") else ()), None)
        again, _ = _kept(c, 6)
        assert all(_same_config(a, b) for (a, _), (b, _) in zip(again, lists[name][0])), name
        assert all(np.array_equal(ra["run"]["res"]["energy_history"], rb["run"]["res"]["energy_history"])
                   for (_, ra), (_, rb) in zip(again, lists[name][0])), name


def test_the_discard_share_is_within_the_cap(lists):
    for name, (out, discarded) in lists.items():
        share = discarded / (len(out) + discarded)
        print(f"[fuzz modes] {name}: {len(out)} kept, {discarded} discarded ({share:.3f} of the draws; cap {fz.DISCARD_CAP:.3f}); smallest "
              f"margins " + ", ".join(f"{k} {min(r['margins'][k] for _, r in out if k in r['margins']):.2e}"
                                      for k in fz.NEAR if any(k in r["margins"] for _, r in out)))
        assert share <= fz.DISCARD_CAP, name
        assert not any(fz.near_ties(r) for _, r in out)


def test_every_kept_configuration_passes_the_headers_refusal_rules(configs):
    for cfg, _ in configs:
        assert fz.check_abi(cfg) == [], fz.describe(cfg)
    # and the checker is no rubber stamp: one violation of each family is named
    cfg = dict(next(c for c, _ in configs if c["dynamics"] == "recombine"))
    for change in (dict(deme=3), dict(n_streams=2), dict(chain_offset=1), dict(every=cfg["T"] + 1), dict(min_pos=cfg["L"]), dict(cuts=[1])):
        assert fz.check_abi(dict(cfg, **change)), change
    # the setter's refusals for a configuration with patterns, and init's free-start rule
    cfg = dict(next(c for c, _ in configs if c.get("patterns") is not None and len(c["patterns"]) == 3))
    pt, L = cfg["patterns"], cfg["L"]
    P = lambda el, ln: motifs.Patterns(np.asarray(el, np.uint32), ln)
    unfree = cfg["start"].copy()
    unfree[-1] = hmot.plant(cfg["wt"], pt, 0, int(np.flatnonzero(motifs.active_mask(pt, L, cfg["wt"], cfg["allow_native"])[0])[0]),
                            np.random.default_rng(0))
    zero = pt.elements.copy()
    zero[1, 0] = 0
    high = pt.elements.copy()
    high[2, int(pt.lengths[2]) - 1] |= 1 << 20
    native = np.zeros((1, 8), np.uint32)
    native[0, 0] = 1 << int(cfg["wt"][0])
    for change in (dict(dynamics="default"), dict(patterns=P(np.ones((33, 8)), [1] * 33)), dict(patterns=P(np.zeros((0, 8)), [])),
                   dict(patterns=P(pt.elements, [0, 1, 1])), dict(patterns=P(np.ones((1, 8)), [9])), dict(patterns=P(zero, pt.lengths)),
                   dict(patterns=P(high, pt.lengths)), dict(patterns=P(np.full((1, 8), (1 << 20) - 1), [1]), allow_native=True),
                   dict(start=unfree)):
        assert fz.check_abi(dict(cfg, **change)), change
    wt_only = dict(cfg, patterns=P(native, [1]), allow_native=False, start=np.where(cfg["start"] == cfg["wt"][0], (cfg["wt"][0] + 1) % 20, cfg["start"]))
    assert not any("forbidden" in w for w in fz.check_abi(wt_only))       # a wild type that is not free is legal without allow_native


def test_the_seed_lists_cover_what_the_hand_picked_cases_leave_alone(lists, configs):
    cfgs = [c for c, _ in configs]
    count = lambda f: sum(1 for c in cfgs if f(c))
    for dyn in fz.DYNAMICS:
        for lib in (False, True):
            k = count(lambda c: c["dynamics"] == dyn and (c["library"] is not None) == lib)
            print(f"[fuzz modes] {dyn}{' + library' if lib else ''}: {k} trials")
            assert k >= 3, (dyn, lib)
        assert count(lambda c: c["dynamics"] == dyn and c["observers"] is not None) >= 1, dyn
    cover = {
        "groups per thread 1": lambda c: fz.groups_per_thread(c["L"]) == 1,
        "groups per thread 2": lambda c: fz.groups_per_thread(c["L"]) == 2,
        "groups per thread 3": lambda c: fz.groups_per_thread(c["L"]) == 3,
        "a range that is not the Potts window": lambda c: (c["min_pos"], c["max_pos"]) != (c["i0"], c["i0"] + c["Lp"] - 1),
        "a range that is the Potts window": lambda c: (c["min_pos"], c["max_pos"]) == (c["i0"], c["i0"] + c["Lp"] - 1),
        "chain_offset != 0": lambda c: c["chain_offset"] != 0,
        "a deme above 64 that is no multiple of 64": lambda c: c.get("deme", 0) > 64 and c["deme"] % 64 != 0,
        "an odd deme": lambda c: c.get("deme", 0) % 2 == 1,
        "more than 64 chains": lambda c: c["n"] > 64,
        "which = 3": lambda c: c["which"] == 3,
        "n_streams > 1 with a library": lambda c: c["n_streams"] > 1 and c["library"] is not None,
        "n_streams > 1 in reversible mode": lambda c: c["n_streams"] > 1 and c["dynamics"] == "reversible",
        "a misaligned cut under recombination": lambda c: c["dynamics"] == "recombine" and any(p % c["every"] for p in np.cumsum(c["cuts"])[:-1]),
        "an aligned cut under recombination": lambda c: c["dynamics"] == "recombine" and len(c["cuts"]) > 1 and not any(p % c["every"] for p in np.cumsum(c["cuts"])[:-1]),
        "a recorder that follows a rung": lambda c: c["observers"] is not None and c["observers"]["rung"] is not None,
    }
    cover.update({f"pas {p}": (lambda c, p=p: c["pas"] == p) for p in (1, 2, 3, 5)})
    cover.update({f"nmut {k}": (lambda c, k=k: c["nmut"] == k) for k in (0, 2, 5)})
    for what, f in cover.items():
        print(f"[fuzz modes] {what}: {count(f)} trials")
        assert count(f) >= 1, what
    happened = {"a mutation cap that is reached": lambda c, r: r["events"]["cap_reached"],
                "an accepted swap": lambda c, r: r["events"].get("accepted_swap"),
                "a replaced slot under a fixed schedule": lambda c, r: c["dynamics"] == "anneal" and r["events"]["replaced_slot"],
                "a replaced slot under the adaptive schedule": lambda c, r: c["dynamics"] == "adaptive" and r["events"]["replaced_slot"],
                "an accepted exchange with differ > 0": lambda c, r: r["events"].get("exchange")}
    for what, f in happened.items():
        k = sum(1 for c, r in configs if f(c, r))
        print(f"[fuzz modes] {what}: {k} trials")
        assert k >= 1, what
    # the PPDE_GRAPH_LEN=4 list replays under every dynamics; in the default environment only recombination has a segment short
    # enough (`every` itself)
    out4 = lists["graph_len_4"][0]
    for dyn in fz.DYNAMICS:
        k = sum(fz.replayed_steps(c, 4) for c, _ in out4 if c["dynamics"] == dyn)
        print(f"[fuzz modes] graph_len_4, {dyn}: {k} replayed steps")
        assert k > 0, dyn
    assert all(fz.replayed_steps(c, 0) == 0 for c, _ in lists["default_env"][0] if c["dynamics"] != "recombine")
    assert any(fz.replayed_steps(c, 0) > 0 for c, _ in lists["default_env"][0] if c["dynamics"] == "recombine")


def test_a_reference_run_equals_itself(configs):
    for cfg, ref in configs:
        assert fz.compare(cfg, ref["run"], ref) == [], fz.describe(cfg)


# helpers_anneal_adaptive's 'target_D' and 'no_shift' change a step only where a deme holds a non-finite energy or energies large
# enough for exp to overflow: no configuration here has either (tests/test_anneal_adaptive_cpu.py plants them on made-up energies)
NOT_PLANTABLE = {("adaptive", "target_D"), ("adaptive", "no_shift")}


@pytest.mark.parametrize("dyn,fault", [(d, f) for d, fs in fz.FAULTS.items() for f in fs if (d, f) not in NOT_PLANTABLE])
def test_the_comparison_reports_every_planted_fault(configs, dyn, fault):
    """The reference run with the fault planted, in the device's layout, against the reference: reported on some kept configuration."""
    tried = 0
    for cfg, ref in configs:
        if cfg["dynamics"] != dyn or (fault.startswith("observers") and cfg["observers"] is None) or \
                (fault == "reverse_library" and cfg["library"] is None):
            continue
        tried += 1
        why = fz.compare(cfg, fz.reference(cfg, fault=fault)["run"], ref)
        if why:
            print(f"[fuzz modes] {dyn}: '{fault}' reported on the {tried}. configuration tried: {why[0]}")
            return
    raise AssertionError(f"'{fault}' was reported on none of {tried} configurations")


def test_the_adaptive_faults_left_out_change_nothing_here(configs):
    for cfg, ref in configs:
        if cfg["dynamics"] == "adaptive":
            for _, fault in sorted(NOT_PLANTABLE):
                assert fault in haa.FAULTS
                assert fz.compare(cfg, fz.reference(cfg, fault=fault)["run"], ref) == [], (fault, fz.describe(cfg))
            return


# ------------------------------------------------------------------------------------------------ the lists with forbidden patterns
def test_the_pattern_lists_cover_what_the_hand_picked_motif_cases_leave_alone(lists, pattern_configs):
    """Asserted on the kept lists and their reference runs alone; every count is printed."""
    count = lambda f: sum(1 for c, r in pattern_configs if f(c, r))

    def show(what, k, least=1):
        print(f"[fuzz modes] patterns: {what}: {k} trials")
        assert k >= least, what

    for name in PATTERN_LISTS:
        out = lists[name][0]
        assert all(c["patterns"] is not None and c["dynamics"] in fz.REVERSIBLE and fz.check_abi(c) == [] for c, _ in out)
        assert all(r["events"]["vetoed"] and r["events"]["accepted_move"] for _, r in out)
        assert all(motifs.is_free(c["start"], c["patterns"], c["wt"], c["allow_native"]).all() for c, _ in out)
        assert all(c["allow_native"] or motifs.is_free(c["wt"][None], c["patterns"], None, False).all() for c, _ in out)
        assert all(len(c["patterns"]) in (1, 3, 32) and 1 <= c["patterns"].lengths.min() and c["patterns"].lengths.max() <= min(8, c["L"])
                   for c, _ in out)
        for dyn in fz.REVERSIBLE:
            for lib in (False, True):
                for native in (False, True):
                    k = sum(1 for c, _ in out if c["dynamics"] == dyn and (c["library"] is not None) == lib and c["allow_native"] == native)
                    print(f"[fuzz modes] {name}: {dyn}{' + library' if lib else ''}, allow_native {native}: {k} trials")
                    assert k >= 1, (name, dyn, lib, native)
    for dyn in fz.REVERSIBLE:
        show(f"{dyn} with the observers on", count(lambda c, r: c["dynamics"] == dyn and c["observers"] is not None))
    for M in (1, 3, 32):
        show(f"{M} patterns", count(lambda c, r: len(c["patterns"]) == M))
    show("vetoed proposals in all", sum(int(r["veto"].sum()) for _, r in pattern_configs))
    facts = [(c, fz.veto_facts(c, r)) for c, r in pattern_configs]
    fact = lambda key, also=lambda c: True: sum(1 for c, f in facts if f[key] and also(c))
    show("a veto whose lowest match starts at p >= 64", fact("start >= 64"))
    show("a veto whose window spans lanes 63 and 64 (a start in 57..63)", fact("window across lanes 63 | 64"))
    show("a veto at the last start L - len", fact("last start"))
    show("a veto whose window holds a frozen residue or one outside [min_pos, max_pos]", fact("context"))
    show("a proposal that matches two or more active patterns", fact("two patterns"))
    show("a veto by a pattern the wild type matches elsewhere under allow_native", fact("native elsewhere"))
    show("a vetoed proposal with exp(log_acc) >= u, inside the cap and not refused", fact("decided by the veto alone"))
    show("a veto directly behind an accepted proposal of the same chain", fact("veto behind an accepted proposal"))
    show("an accepted proposal directly behind a veto of the same chain", fact("accepted behind a veto"))
    for pas in (1, 5):
        show(f"a veto under pas {pas}", count(lambda c, r: c["pas"] == pas and r["veto"].any()))
    for g in (2, 3):
        show(f"{g} logit groups per thread", count(lambda c, r: fz.groups_per_thread(c["L"]) == g))
    show("chain_offset != 0", count(lambda c, r: c["chain_offset"] != 0))
    show("n_streams > 1 with a share that is no multiple of four", count(lambda c, r: c["n_streams"] > 1 and fz.ragged_share(c["n"], c["n_streams"])))
    assert all(fz.ragged_share(c["n"], c["n_streams"]) for c, _ in pattern_configs if c["n_streams"] > 1)
    show("a deme of 70", count(lambda c, r: c.get("deme") == 70))
    show("a proposal range that is not the Potts window", count(lambda c, r: (c["min_pos"], c["max_pos"]) != (c["i0"], c["i0"] + c["Lp"] - 1)))
    show("a run cut into several calls", count(lambda c, r: len(c["cuts"]) > 1))
    for k in (0, 2, 5):
        show(f"nmut {k}", count(lambda c, r, k=k: c["nmut"] == k))
    show("outcome 4 under recombination", fact("outcome 4"))
    show("a veto behind a replaced slot under a fixed schedule", fact("veto behind a replaced slot", lambda c: c["dynamics"] == "anneal"))
    show("a veto behind a replaced slot under the adaptive schedule", fact("veto behind a replaced slot", lambda c: c["dynamics"] == "adaptive"))
    show("a veto on a chain that has just swapped rungs", fact("veto behind a swap"))
    out4 = lists["patterns_graph_len_4"][0]
    for dyn in fz.REVERSIBLE:
        k = sum(fz.replayed_steps(c, 4) for c, _ in out4 if c["dynamics"] == dyn)
        print(f"[fuzz modes] patterns_graph_len_4, {dyn}: {k} replayed steps")
        assert k > 0, dyn


# 'veto_through_u' (the veto as -inf in the ratio) accepts a vetoed proposal only where u is exactly 0, one draw in 2^24
MOTIF_NOT_PLANTABLE = ("veto_through_u",)


def _applies(fault, cfg):
    return {"one_child_only": cfg["dynamics"] == "recombine", "children_counted": cfg["dynamics"] == "recombine",
            "native_per_pattern": cfg["allow_native"], "frozen_not_context": True}.get(fault, True)


@pytest.mark.parametrize("fault", [f for f in fz.MOTIF_FAULTS if f not in MOTIF_NOT_PLANTABLE])
def test_the_comparison_reports_every_planted_motif_fault(pattern_configs, fault):
    """The constrained reference with the fault planted, in the device's layout, against the reference: reported on some kept
    configuration with patterns."""
    assert set(hmot.FAULTS) | set(hmot.RUN_FAULTS) == set(fz.MOTIF_FAULTS)
    tried = 0
    for cfg, ref in pattern_configs:
        if not _applies(fault, cfg):
            continue
        tried += 1
        why = fz.compare(cfg, fz.reference(cfg, fault=fault)["run"], ref)
        if why:
            print(f"[fuzz modes] patterns, {cfg['dynamics']}: '{fault}' reported on the {tried}. configuration tried: {why[0]}")
            return
    raise AssertionError(f"'{fault}' was reported on none of {tried} configurations")


def test_the_motif_fault_left_out_changes_nothing_here(pattern_configs):
    for cfg, ref in pattern_configs:
        assert all((nz[2].numpy() > 0).all() for nz in ref["noise"]), fz.describe(cfg)      # no accept uniform is exactly 0
    for cfg, ref in pattern_configs[::5]:
        for fault in MOTIF_NOT_PLANTABLE:
            assert fz.compare(cfg, fz.reference(cfg, fault=fault)["run"], ref) == [], (fault, fz.describe(cfg))

"""The mode fuzzer without a GPU (tests/helpers_fuzz_modes.py; the GPU side is tests/fuzz_modes.py under tests/test_fuzz_modes_gpu.py):
the seed lists the GPU module runs are a pure function of their seeds, discard at most one draw in eight, hold only configurations
the C ABI accepts, cover the axes the hand-picked mode tests leave alone, and the one comparison both sides call reports every fault
the reference runners know how to plant."""
import numpy as np
import pytest

import helpers_anneal_adaptive as haa
import helpers_fuzz_modes as fz


@pytest.fixture(scope="module")
def lists():
    return {name: fz.kept(c["seed"], c["trials"], c["dynamics"], c.get("graph_len", 0)) for name, c in fz.GPU_CASES.items()}


@pytest.fixture(scope="module")
def configs(lists):
    return [pair for out, _ in lists.values() for pair in out]


def _same_config(a, b):
    return fz.describe(a) == fz.describe(b) and np.array_equal(a["start"], b["start"]) and np.array_equal(a["wt"], b["wt"]) and \
        (a["library"] is None) == (b["library"] is None) and (a["library"] is None or np.array_equal(a["library"], b["library"]))


def test_the_kept_lists_are_a_pure_function_of_the_seed(lists):
    """Drawn again from scratch (references and discards included), the first six kept configurations of every list are the same."""
    for name, c in fz.GPU_CASES.items():
        fz._KEPT.pop((c["seed"], 6, c["dynamics"], c.get("graph_len", 0)), None)
        again, _ = fz.kept(c["seed"], 6, c["dynamics"], c.get("graph_len", 0))
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

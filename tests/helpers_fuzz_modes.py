"""The mode fuzzer's generator, reference and comparison (tests/fuzz_modes.py on the GPU, tests/test_fuzz_modes_cpu.py without one).

`draw(rng)` makes one configuration of the chain modes at a random geometry as a plain dict: default, reversible, tempering,
annealing (fixed and adaptive) and recombination, each with and without a design library, with the observers on half the draws,
over the axes the hand-picked mode tests leave alone (two and three logit groups per thread, padded state rows of any length, a
proposal range that is not the Potts window, demes astride 64 lanes, pas 1 and 5, several streams, a run cut into several calls).
With `forbid` the configuration also carries forbidden patterns (ppde_chains_set_forbidden_patterns) under one of the five
reversible dynamics, built around proposals its own unconstrained reference accepted (`_patterns`).
`check_abi(cfg)` restates the refusal rules of include/ppde_hip.h for such a dict; `draw` returns only what passes them.

`reference(cfg)` is the CPU run of the configuration: orc.device_noise restates the device RNG, the mode's own helper runs the
iterations, the observers' rules (helpers_archive, helpers_stats, helpers_pairs, the recorder's row rule of ppde_amd.sampler) turn
its states into what the device must hold. It is returned in the layout a device run is read in, with the reference's own
near-tie margins. No rule is stated here a second time: the veto is helpers_motifs' constrained iteration inside each mode's helper.

`compare(cfg, run, ref)` is the ONE comparison both modules call: the GPU script hands it a device run, the CPU module a reference
run with a planted fault. No chain is exempt: `kept(...)` keeps a draw only if every decision of its reference run is clear of a
near-tie by the thresholds the mode's own replay test applies (NEAR), and replaces a discarded draw by the next one of the same
stream, so the kept list is a pure function of the seed. Every tolerance is imported from the mode helpers."""
import contextlib

import numpy as np
import torch

import helpers_anneal as ha
import helpers_anneal_adaptive as haa
import helpers_archive as har
import helpers_library as hl
import helpers_modes as hm
import helpers_motifs as hmot
import helpers_pairs as hp
import helpers_recombine as hrc
import helpers_reversible as hr
import helpers_stats as hs
import helpers_tempering as ht
import ppde_oracle as orc
from helpers import oracle_energy
from ppde_amd import library as dl
from ppde_amd import motifs
from ppde_amd import synthetic
from ppde_amd.sampler import recorder_row_of, recorder_rows

A = 20
BLOCK = 512                                    # threads of a chain workgroup (PPDE_BLOCK): groups per thread = ceil(L * 20 / 4 / 512)
DYNAMICS = ("default", "reversible", "tempering", "anneal", "adaptive", "recombine")
GROUPED = ("tempering", "anneal", "adaptive", "recombine")
REVERSIBLE = DYNAMICS[1:]                       # the dynamics forbidden patterns compose with
# the seeds of the two pattern lists, searched on the CPU reference alone for lists that show every item
# tests/test_fuzz_modes_cpu.py asserts of them
PATTERN_SEEDS = (8, 3)
# the thresholds of the modes' own replay tests: swap |d - log u| (tests/test_tempering_cpu.py), selection |tau - C| / W
# (tests/test_anneal_gpu.py), recombination |exp(d) - u| (tests/test_recombine_gpu.py); race gap and accept margin are helpers_modes'
NEAR = dict(gap=hm.GAP_TOL, accept=hm.ACC_TOL, swap=2e-3, select=1e-4, cross=1e-4)
PLAN_REL = 1e-12                               # tests/test_anneal_gpu.py: log_mean_w and ess against helpers_anneal.plan, relative
DISCARD_CAP = 1.0 / 8.0                        # at most this share of a seed list's draws may be discarded
# what tests/test_fuzz_gpu.py runs: one child process each, in this order
GPU_CASES = {
    "default_env": dict(seed=43, trials=24, env={}, dynamics=None),
    "graph_len_4": dict(seed=53, trials=24, env={"PPDE_GRAPH_LEN": "4"}, dynamics=None, graph_len=4),
    "general_kernels": dict(seed=33, trials=8, env={"PPDE_CHAIN_SPEC": "0"}, dynamics=("default",)),
    "patterns": dict(seed=PATTERN_SEEDS[0], trials=20, env={"FZ_FORBID": "1"}, dynamics=REVERSIBLE, forbid=True),
    "patterns_graph_len_4": dict(seed=PATTERN_SEEDS[1], trials=20, env={"FZ_FORBID": "1", "PPDE_GRAPH_LEN": "4"}, dynamics=REVERSIBLE,
                                 graph_len=4, forbid=True),
}


def groups_per_thread(L):
    return (L * A // 4 + BLOCK - 1) // BLOCK


# ------------------------------------------------------------------------------------------------ the generator
def _library(rng, wt, L, lo, hi):
    """A seeded library over the range widened by up to three residues on each side (so that the range mask and the library both
    bind), with an open residue inside the range."""
    w_lo, w_hi = max(0, lo - int(rng.integers(0, 4))), min(L - 1, hi + int(rng.integers(0, 4)))
    base = int(rng.integers(1, 1 << 30))
    for k in range(64):
        try:
            lib = hl.seeded_library(wt, w_lo, w_hi, seed=base + k)
        except AssertionError:
            continue
        if lib[lo:hi + 1].any():
            return lib
    raise AssertionError("no library for this range")


def draw(rng, dynamics=None, library=None, graph_len=0, forbid=False, allow_native=True):
    """One configuration. `dynamics` / `library` pin those two axes (kept() cycles through them); everything else is drawn.
    `graph_len`: the run is to replay graph segments of that length (PPDE_GRAPH_LEN): graphs are on, a recombination `every` divides
    it, and the cuts are drawn again until some call replays a segment.
    `forbid`: a configuration with forbidden patterns (`patterns`, `allow_native`): one of the REVERSIBLE dynamics, with several
    streams a population some stream's share of which is no multiple of the veto kernel's four chains per workgroup, and patterns
    built on the configuration's own unconstrained reference (`_patterns`); None where none could be built. Without it nothing new
    is drawn and no variate consumed."""
    if forbid and dynamics is None:
        dynamics = REVERSIBLE[int(rng.integers(len(REVERSIBLE)))]
    dyn = DYNAMICS[int(rng.integers(len(DYNAMICS)))] if dynamics is None else dynamics
    with_lib = bool(rng.integers(2)) if library is None else bool(library)
    with_cnn = bool(rng.integers(0, 5) == 0)                               # (the CPU CNN is slow: a minority, at L <= 100)
    L = int(rng.integers(12, 101 if with_cnn else 261))
    Lp = int(rng.integers(4, L + 1))
    i0 = int(rng.integers(0, L - Lp + 1))
    lamda = float(rng.choice([0.5, 5.0])) if with_cnn else 0.0
    min_pos = int(rng.integers(0, L // 2))
    max_pos = int(rng.integers(min_pos, L))
    if rng.integers(0, 3) == 0:
        min_pos, max_pos = i0, i0 + Lp - 1
    if with_lib and max_pos - min_pos < 2:                                 # (room for an open and a frozen residue)
        max_pos = min_pos + 2
    wt = rng.integers(0, A, L).astype(np.uint8)
    pas = int(rng.choice([1, 2, 3, 5]))
    nmut = int(rng.choice([0, 2, 5]))
    cfg = dict(dynamics=dyn, L=L, Lp=Lp, i0=i0, which=3 if with_cnn else 1, lamda=lamda, potts_seed=int(rng.integers(0, 1000)),
               min_pos=min_pos, max_pos=max_pos, wt=wt, pas=pas, nmut=nmut, seed=int(rng.integers(1, 1 << 31)),
               library=_library(rng, wt, L, min_pos, max_pos) if with_lib else None,
               reuse_grad=bool(rng.integers(2)), use_graph=bool(rng.integers(2)))
    # population: a multiple of the mode's group, 4..40 chains or one value above 64
    big = bool(rng.integers(0, 8) == 0)
    group = 1
    if dyn == "tempering":
        R = int(rng.choice([2, 3, 4]))
        group = R
        cfg.update(betas=tuple(ht.REPLAY_BETAS[:R]), swap_every=int(rng.choice([1, 2, 3])))
    elif dyn in ("anneal", "adaptive"):
        # (a deme of 70 is rare: its selection has D^2 breakpoints, and most such draws sit within 1e-4 of one and are discarded)
        group = int(rng.choice([2, 3, 4, 6, 8, 70], p=[0.184, 0.184, 0.184, 0.184, 0.184, 0.08]))
        cfg.update(deme=group, every=int(rng.choice([1, 2, 3])))
    elif dyn == "recombine":
        group = int(rng.choice([2, 4, 6, 8, 70]))                          # (the setter refuses an odd deme)
        cfg.update(deme=group, every=int(rng.choice([k for k in (1, 2, 3) if not graph_len or graph_len % k == 0])))
    if group == 70:
        n = 70
    elif big:
        n = group * (64 // group + 1) + (5 if group == 1 else 0)           # 69 chains, or the multiple of the group above 64
    else:
        lo_k, hi_k = -(-4 // group), max(40 // group, 1)
        if dyn == "adaptive":
            hi_k = min(hi_k, max(lo_k, 3))                                 # (its reference reruns the prefix deme by deme)
        n = group * int(rng.integers(lo_k, hi_k + 1))
    T = 6 if n > 64 else int(rng.integers(6, 15))
    cfg.update(n=n, T=T, chain_offset=group * int(rng.integers(1, 50)) if rng.integers(2) else 0)
    # (a deme of 70 takes one event: the selection has D^2 breakpoints, and every further event doubles the near-ties discarded)
    if dyn == "anneal":
        S = int(rng.integers(1, 5)) if group != 70 else 1
        mid = np.sort(rng.choice(ha.REPLAY_BETAS, S - 1)).tolist()
        cfg["schedule"] = tuple([ha.REPLAY_BETAS[0]] + mid + [ha.REPLAY_BETAS[-1]])
    if dyn == "adaptive":
        cfg.update(beta_start=ha.REPLAY_BETAS[0], beta_end=ha.REPLAY_BETAS[-1], ess_target=float(rng.choice([0.3, 0.5, 0.9], p=[0.2, 0.2, 0.6])),   # (below 0.9 most steps jump to the end)
                   min_step=float(rng.choice([2.0 ** -12, 2.0 ** -2])), max_stages=int(rng.integers(2, 5)) if group != 70 else 1)
    # observers on half the draws, all four together
    cfg["observers"] = None
    if rng.integers(2):
        every = int(rng.choice([1, 2, 3]))
        rung = int(rng.integers(0, len(cfg["betas"]))) if dyn == "tempering" and rng.integers(2) else None
        cfg["observers"] = dict(every=every, burn_in=int(rng.integers(0, T - every + 1)), rung=rung, K=int(rng.choice([1, 3, 32])),
                                sites=hp.scattered_sites(L, int(rng.choice([s for s in hp.SITE_COUNTS if s <= L])), int(rng.integers(1 << 20))))
    cfg["n_streams"] = int(rng.choice([1, 2, 3])) if dyn in ("default", "reversible") and cfg["observers"] is None else 1
    if forbid and cfg["n_streams"] > 1 and not ragged_share(n, cfg["n_streams"]):
        n = cfg["n"] = n + 1
    # the run, cut into 1..4 calls; with recombination on half the draws at multiples of `every` only
    if graph_len:
        cfg["use_graph"] = True
    for attempt in range(16):
        pieces = int(rng.integers(1, 5)) if attempt < 15 else 1
        places = np.arange(1, T)
        if dyn == "recombine" and rng.integers(2):
            places = places[places % cfg["every"] == 0]
        at = np.sort(rng.choice(places, size=min(pieces - 1, places.size), replace=False)).tolist() if places.size else []
        cfg["cuts"] = [int(b - a) for a, b in zip([0] + at, at + [T])]
        if not graph_len or replayed_steps(cfg, graph_len) > 0:
            break
    # distinct random start states inside the proposal range and the library
    words = dl.full_library(L) if cfg["library"] is None else cfg["library"]
    span = np.array([l for l in range(min_pos, max_pos + 1) if words[l]])
    start = np.tile(wt, (n, 1))
    for b in range(n):
        k = min(b % 5, span.size, nmut - 1 if nmut else 5)                 # (inside the cap: the support of the reversible law)
        for l in rng.choice(span, size=k, replace=False):
            start[b, l] = rng.choice(np.flatnonzero((int(words[l]) >> np.arange(A)) & 1))
    cfg["start"] = start
    if forbid:
        assert dyn in REVERSIBLE
        cfg["allow_native"] = bool(allow_native)
        cfg["patterns"] = _patterns(rng, cfg, reference(cfg))
        if cfg["patterns"] is None:
            return None
    assert not check_abi(cfg), check_abi(cfg)
    return cfg


def stream_shares(n, n_streams):
    """The chains of every stream's sub-population (ppde_chains_create: at most 8 streams, the remainder to the first ones)."""
    K = min(n_streams, 8, n) if n_streams > 1 else 1
    return [n // K + (k < n % K) for k in range(K)]


def ragged_share(n, n_streams):
    return any(s % 4 for s in stream_shares(n, n_streams))


def _extras(rng, density, without=()):
    w = int(sum(1 << k for k in range(A) if rng.random() < density))
    for k in without:
        w &= ~(1 << int(k))
    return w


def _patterns(rng, cfg, ref0):
    """Patterns for `cfg` from its unconstrained reference run `ref0`: M of {1, 3, 32}, each built around the mutated residue of a
    proposal that run ACCEPTED (pattern 0 around one of the four earliest: up to its first veto the constrained run is the unconstrained one,
    so that proposal is made again and only the veto can reject it) -- the element at that residue holds the proposal's letter and neither
    the current nor the wild-type one, the others the proposal's letters in a window of the drawn length, each with random extra
    letters; on a third of the draws each the window sits at the last start (around a move among the last eight residues, where
    the run has one) or across lane 64 of the veto kernel, where it can. Under
    recombination every other pattern is built on an accepted child instead, over a residue it took from its partner and one it
    kept. Every pattern is drawn again until the starts (without allow_native: and the wild type) are free of it."""
    L, wt, n, T = cfg["L"], cfg["wt"].astype(np.int64), cfg["n"], cfg["T"]
    native = cfg["allow_native"]
    M = int(rng.choice([1, 3, 32]))
    states, props = ref0["states"], ref0["proposals"]
    acc = ref0["run"]["tr"]["accepted"].astype(bool)
    moves = [(int(t), int(b)) for t, b in zip(*np.nonzero(acc)) if (props[t, b] != states[t, b]).any()]          # in time order
    kids = []
    if cfg["dynamics"] == "recombine":
        rc = ref0["run"]["recomb"]
        for e, b in zip(*np.nonzero((rc["outcome"] == 1) & (rc["differ"] > 0))):
            own, other = ref0["pre_event"][e][b], ref0["pre_event"][e][rc["partner"][e, b]]
            child = states[(e + 1) * cfg["every"], b]
            s1, s2 = np.flatnonzero(child != own), np.flatnonzero(child != other)
            near = [(int(a), int(c)) for a in s1 for c in s2 if abs(int(a) - int(c)) <= 7]
            if near:
                kids.append((child, own, other, near))
    if not moves:
        return None
    tail = [(t, b) for t, b in moves if (props[t, b] != states[t, b])[max(0, L - 8):].any()]
    el, ln = np.zeros((M, 8), np.uint32), np.zeros(M, np.int32)
    twin = None
    for m in range(M):
        for attempt in range(60):
            words = np.zeros(8, np.uint32)
            if kids and m % 2 == 1:
                child, own, other, near = kids[int(rng.integers(len(kids)))]
                a, c = near[int(rng.integers(len(near)))]
                lo_s, hi_s = min(a, c), max(a, c)
                k = int(rng.integers(hi_s - lo_s + 1, min(8, L) + 1))
                p = int(rng.integers(max(0, hi_s - k + 1), min(lo_s, L - k) + 1))
                for j in range(k):
                    words[j] = (1 << int(child[p + j])) | _extras(rng, 0.3)
                words[a - p] = (1 << int(child[a])) | _extras(rng, 0.2, (own[a],))
                words[c - p] = (1 << int(child[c])) | _extras(rng, 0.2, (other[c],))
            else:
                where = int(rng.integers(3))
                if m == 1 and twin is not None and attempt == 0:
                    t, b = twin                                                 # a second pattern on the first one's proposal
                elif m > 0 and where == 0 and tail:
                    t, b = tail[int(rng.integers(len(tail)))]                   # a move among the last eight residues
                else:
                    t, b = moves[int(rng.integers(min(len(moves), 4 if m == 0 and attempt < 20 else len(moves))))]
                if m == 0:
                    twin = (t, b)
                x, y = states[t, b], props[t, b]
                l = int(np.flatnonzero(x != y)[-1]) if where == 0 else int(rng.choice(np.flatnonzero(x != y)))
                k = int(rng.integers(L - l if where == 0 and L - l <= min(8, L) else 1, min(8, L) + 1))
                lo_p, hi_p = max(0, l - k + 1), min(l, L - k)
                p = int(rng.integers(lo_p, hi_p + 1))
                if where == 0 and hi_p == L - k:
                    p = L - k
                seam = [s for s in range(lo_p, hi_p + 1) if s < 64 <= s + k - 1]
                if where == 1 and seam:
                    p = int(rng.choice(seam))
                wide = float(rng.choice([0.15, 0.5, 1.0]))
                for j in range(k):
                    words[j] = (1 << int(y[p + j])) | _extras(rng, wide)
                words[l - p] = (1 << int(y[l])) | _extras(rng, 0.2, (x[l], wt[l]))
            one = motifs.Patterns(words[None], [k])
            if motifs.is_free(cfg["start"], one, wt, native).all() and (native or motifs.is_free(wt[None], one, None, False).all()):
                el[m], ln[m] = words, k
                break
        else:
            return None
    pt = motifs.Patterns(el, ln)
    return pt if motifs.active_mask(pt, L, wt, native).any() else None


def check_abi(cfg):
    """The refusals of include/ppde_hip.h that concern such a configuration, as a list of violated rules (empty: accepted)."""
    bad = []
    L, n, T, dyn, off = cfg["L"], cfg["n"], cfg["T"], cfg["dynamics"], cfg["chain_offset"]

    def need(ok, what):
        if not ok:
            bad.append(what)

    need(5 <= L <= 307, "L outside 5..307 for ppde_chains")
    need(1 <= cfg["Lp"] <= min(L, 512) and 0 <= cfg["i0"] and cfg["i0"] + cfg["Lp"] <= L, "Potts window")
    need(1 <= cfg["pas"] <= 64 and cfg["nmut"] >= 0 and n >= 1 and off + n < 2 ** 32, "ppde_chain_config")
    need(0 <= cfg["min_pos"] <= cfg["max_pos"] < L, "bad [min_pos, max_pos]")
    need(cfg["which"] in (1, 3), "which")
    need(sum(cfg["cuts"]) == T and all(k >= 1 for k in cfg["cuts"]), "the cuts are not the run")
    lib = cfg["library"]
    if lib is not None:
        need((lib < (1 << A)).all(), "library: a bit >= 20")
        opened = np.flatnonzero(lib)
        need(((lib[opened] >> cfg["wt"][opened].astype(np.uint32)) & 1).all(), "library: an open residue lacks its wild-type letter")
        need(lib[cfg["min_pos"]:cfg["max_pos"] + 1].any(), "library: no residue of the range is open")
    single = cfg["n_streams"] <= 1
    if dyn == "tempering":
        b = np.asarray(cfg["betas"], np.float32)
        need(1 <= b.size <= 64 and np.isfinite(b).all() and (b > 0).all() and (b[1:] < b[:-1]).all(), "ladder")
        need(cfg["swap_every"] >= 0 and n % b.size == 0 and off % b.size == 0 and single, "tempering: groups or streams")
    if dyn in ("anneal", "adaptive"):
        D = cfg["deme"]
        need(2 <= D <= 1024 and n % D == 0 and off % D == 0 and cfg["every"] >= 1 and single, "annealing: deme, every or streams")
    if dyn == "anneal":
        s = np.asarray(cfg["schedule"], np.float32)
        need(1 <= s.size - 1 <= 4096 and np.isfinite(s).all() and (s > 0).all() and (s[1:] >= s[:-1]).all(), "schedule")
        need(ha.events_cap(s.size - 1, T, cfg["every"]) >= 1, "annealing: no event fits")
    if dyn == "adaptive":
        b0, b1, rho, step = (np.float32(cfg[k]) for k in ("beta_start", "beta_end", "ess_target", "min_step"))
        need(1 <= cfg["max_stages"] <= 4096 and 0 < b0 < b1 < np.inf and 0 < rho < 1, "adaptive annealing: stages, betas or target")
        need(np.isfinite(step) and step >= b1 * np.float32(2.0 ** -20), "adaptive annealing: min_step")
        need(min(cfg["max_stages"], T // cfg["every"]) >= 1, "adaptive annealing: no event fits")
    if dyn == "recombine":
        D = cfg["deme"]
        need(D >= 2 and D % 2 == 0 and n % D == 0 and off % D == 0 and cfg["every"] >= 1 and T // cfg["every"] >= 1 and single,
             "recombination: deme, every or streams")
        need(hrc.open_list(L, cfg["min_pos"], cfg["max_pos"], lib).size >= 1, "recombination: no open residue")
    ob = cfg["observers"]
    if ob is not None:
        need(single, "observers with n_streams > 1")
        need(ob["every"] >= 1 and ob["burn_in"] >= 0 and recorder_rows(T, ob["burn_in"], ob["every"]) >= 1, "recorder: no row fits")
        need(ob["rung"] is None or (dyn == "tempering" and 0 <= ob["rung"] < len(cfg["betas"])), "recorder: rung")
        s = np.asarray(ob["sites"])
        need(1 <= s.size <= L and s[0] >= 0 and s[-1] < L and (np.diff(s) > 0).all(), "pair sites")
        need(1 <= ob["K"] <= 32, "archive k")
    pt = cfg.get("patterns")
    if pt is not None:                                                      # ppde_chains_set_forbidden_patterns, and init's free starts
        need(dyn != "default", "forbidden patterns need reversible mode")
        need(1 <= len(pt) <= motifs.MAX_PATTERNS, "forbidden patterns: n_patterns outside 1..32")
        need(all(1 <= int(k) <= min(motifs.MAX_LEN, L) for k in pt.lengths), "forbidden patterns: a length outside 1..8 or above L")
        need(all(0 < int(pt.elements[m, j]) < (1 << A) for m in range(len(pt)) for j in range(min(int(pt.lengths[m]), motifs.MAX_LEN))),
             "forbidden patterns: an element that is 0 or has a bit >= 20")
        if not bad:
            need(motifs.active_mask(pt, L, cfg["wt"], cfg["allow_native"]).any(), "forbidden patterns: no active (m, p)")
            need(motifs.is_free(cfg["start"], pt, cfg["wt"], cfg["allow_native"]).all(), "forbidden patterns: a start that is not free")
    if dyn != "default" and lib is not None:                                # reversible mode: a start inside the library
        try:
            dl.check_population(lib, cfg["start"])
        except ValueError as e:
            bad.append(str(e))
    return bad


def describe(cfg):
    ob = cfg["observers"]
    extra = {"tempering": lambda: f" betas={cfg['betas']} swap_every={cfg['swap_every']}",
             "anneal": lambda: f" D={cfg['deme']} every={cfg['every']} schedule={cfg['schedule']}",
             "adaptive": lambda: f" D={cfg['deme']} every={cfg['every']} ess={cfg['ess_target']} min_step={cfg['min_step']} stages={cfg['max_stages']}",
             "recombine": lambda: f" D={cfg['deme']} every={cfg['every']}"}.get(cfg["dynamics"], lambda: "")()
    if cfg.get("patterns") is not None:
        extra += f" patterns={len(cfg['patterns'])} (lengths {sorted(set(cfg['patterns'].lengths.tolist()))}) native={cfg['allow_native']}"
    return (f"{cfg['dynamics']}{'+lib' if cfg['library'] is not None else ''}{extra} L={cfg['L']} Lp={cfg['Lp']} i0={cfg['i0']} "
            f"pos=[{cfg['min_pos']},{cfg['max_pos']}] which={cfg['which']} lam={cfg['lamda']} n={cfg['n']} off={cfg['chain_offset']} T={cfg['T']} "
            f"cuts={cfg['cuts']} pas={cfg['pas']} nmut={cfg['nmut']} reuse={cfg['reuse_grad']} graph={cfg['use_graph']} "
            f"streams={cfg['n_streams']} seed={cfg['seed']} observers="
            + ("off" if ob is None else f"(every {ob['every']} burn_in {ob['burn_in']} rung {ob['rung']} S {len(ob['sites'])} K {ob['K']})"))


def model_parts(cfg):
    """(J, h, cnn states or None) of a configuration's synthetic experts."""
    J, h = synthetic.make_potts(cfg["Lp"], seed=cfg["potts_seed"])
    cnn = [synthetic.make_cnn_state(cfg["L"], s) for s in range(3)] if cfg["which"] & 2 else None
    return J, h, cnn


def segment_lengths(cfg, graph_len):
    """The graph segments ppde_chains_init captures for such a run (include/ppde_hip.h, ppde_chains_graph_stats and the
    recombination paragraph): PPDE_GRAPH_LEN or (100, 20); with recombination multiples of `every` only; each only if it fits."""
    if not cfg["use_graph"]:
        return []
    if cfg["dynamics"] != "recombine":
        lens = [graph_len] if graph_len else [100, 20]
    else:
        every = cfg["every"]
        lens = ([graph_len] if graph_len % every == 0 else []) if graph_len else sorted({every * (100 // every), every}, reverse=True)
    return [k for k in lens if k <= cfg["T"]]


def replayed_steps(cfg, graph_len=0):
    """Iterations the cut plan replays from graphs: per call the longest segment that fits, as often as it fits -- with
    recombination only from positions that are multiples of `every`, the iterations up to the next one issued eagerly."""
    lens = segment_lengths(cfg, graph_len)
    every = cfg["every"] if cfg["dynamics"] == "recombine" and lens else 1
    pos, replayed = 0, 0
    for steps in cfg["cuts"]:
        done = 0
        while done < steps:
            left = steps - done
            seg = next((k for k in lens if k <= left), None) if (pos + done) % every == 0 else None
            if seg:
                replayed += seg
                done += seg
            else:
                done += left if (pos + done) % every == 0 else min(left, every - (pos + done) % every)
        pos += steps
    return replayed


# ------------------------------------------------------------------------------------------------ the reference
def _np(x):
    return x.numpy() if torch.is_tensor(x) else np.asarray(x)


@contextlib.contextmanager
def library_ignored_on_the_reverse_path():
    """A planted fault: inside the block helpers_reversible's reverse rows (the second gradient of every iteration) take no library."""
    real, seen = hr.proposal_row, dict(last=None, flips=0)

    def row(grad, state, wt_idx, min_pos, max_pos, thr, forbid):
        if grad is not seen["last"]:
            seen["last"], seen["flips"] = grad, seen["flips"] + 1
        return real(grad, state, wt_idx, min_pos, max_pos, thr, torch.zeros_like(forbid) if seen["flips"] % 2 == 0 else forbid)

    hr.proposal_row = row
    try:
        yield
    finally:
        hr.proposal_row = real


MOTIF_FAULTS = hmot.FAULTS + hmot.RUN_FAULTS      # planted in a configuration with patterns, under any of the REVERSIBLE dynamics
FAULTS = {"reversible": ("reverse_library",),
          "tempering": ("swap_u_shifted", "beta_on_rows_only"),
          "anneal": ha.FAULTS + ("observers_before_selection",),
          "adaptive": haa.FAULTS,
          "recombine": ("round0", "observers_before_event")}


def _runner(cfg, energy, x0, noise, fault):
    """The mode's CPU run of all chains (adaptive annealing: deme by deme) with traces and forward rows."""
    dyn, lib, wt = cfg["dynamics"], cfg["library"], cfg["wt"]
    fn = lambda t: noise[t]
    common = (fn, cfg["T"], cfg["min_pos"], cfg["max_pos"], cfg["pas"], cfg["nmut"])
    seed, off = cfg["seed"], cfg["chain_offset"]
    forb = {}
    if cfg.get("patterns") is not None:                                     # the mode's helper runs its iteration under the constraint
        forb = dict(forbidden=(cfg["patterns"], cfg["allow_native"]), motif_fault=fault if fault in MOTIF_FAULTS else None)
    if dyn == "default":
        if lib is None:
            return [orc.run(energy, x0, wt, *common, False, trace=True, keep_probs=True)]
        return [hl.masked_run(lib, energy, x0, wt, *common, False, trace=True, keep_probs=True)]
    if dyn == "reversible":
        with library_ignored_on_the_reverse_path() if fault == "reverse_library" else contextlib.nullcontext():
            if forb:
                return [hmot.constrained_run(energy, x0, wt, *common, lib, cfg["patterns"], cfg["allow_native"], forb["motif_fault"],
                                             keep_probs=True)]
            return [hr.reversible_run(energy, x0, wt, *common, trace=True, keep_probs=True, allowed=lib)]
    if dyn == "tempering":
        R = len(cfg["betas"])
        first = off + np.arange(cfg["n"] // R) * R
        swap_u = (lambda it: ht.swap_uniforms(seed, first, it + 1, R)) if fault == "swap_u_shifted" else None
        with hm.beta_on_rows_only() if fault == "beta_on_rows_only" else contextlib.nullcontext():
            return [ht.tempered_run(energy, x0, wt, *common, cfg["betas"], cfg["swap_every"], seed=seed, chain_offset=off, allowed=lib,
                                    trace=True, keep_probs=True, swap_u=swap_u, **forb)]
    if dyn == "anneal":
        return [ha.annealed_run(energy, x0, wt, *common, cfg["schedule"], cfg["every"], cfg["deme"], seed=seed, chain_offset=off,
                                allowed=lib, trace=True, keep_probs=True, fault=fault if fault in ha.FAULTS else None, **forb)]
    if dyn == "adaptive":
        D, out = cfg["deme"], []
        for d in range(cfg["n"] // D):
            sl = slice(d * D, (d + 1) * D)
            sub = lambda t, sl=sl: (noise[t][0][sl], noise[t][1][:, sl], noise[t][2][sl])
            out.append(haa.adaptive_run(energy, x0[sl], wt, sub, cfg["T"], cfg["min_pos"], cfg["max_pos"], cfg["pas"], cfg["nmut"],
                                        cfg["beta_start"], cfg["beta_end"], cfg["ess_target"], cfg["min_step"], cfg["every"], D,
                                        max_stages=cfg["max_stages"], seed=seed, chain_offset=off + d * D, allowed=lib,
                                        fault=fault if fault in haa.FAULTS else None, trace=True, keep_probs=True, **forb))
        return out
    words = dl.full_library(cfg["L"]) if lib is None else lib
    return [hrc.recombined_run(energy, x0, wt, *common, cfg["every"], cfg["deme"], seed, words, chain_offset=off,
                               fault="round0" if fault == "round0" else None, trace=True, keep_probs=True, **forb)]


def _observers(cfg, peeks, accepted, U, rung_hist):
    """What the four observers hold after the run whose population after t iterations is peeks[t]: their own rules."""
    ob, T, n, L = cfg["observers"], cfg["T"], cfg["n"], cfg["L"]
    R = len(cfg["betas"]) if cfg["dynamics"] == "tempering" else 0
    rows = [t for t in range(1, T + 1) if recorder_row_of(t, ob["burn_in"], ob["every"]) is not None]
    assert [recorder_row_of(t, ob["burn_in"], ob["every"]) for t in rows] == list(range(recorder_rows(T, ob["burn_in"], ob["every"])))
    if ob["rung"] is None:
        chain = np.tile(np.arange(n, dtype=np.int32), (len(rows), 1))
    else:                                                                  # one slot per ensemble: the chain that holds the rung after the swap
        chain = np.stack([np.flatnonzero(rung_hist[t] == ob["rung"]) for t in rows]).astype(np.int32)
    rec = dict(rows=len(rows), chain=chain, idx=np.stack([peeks[t]["idx"][chain[r]] for r, t in enumerate(rows)]),
               energy=np.stack([peeks[t]["energy"][chain[r]] for r, t in enumerate(rows)]),
               fitness=np.stack([peeks[t]["fitness"][chain[r]] for r, t in enumerate(rows)]))
    rec["site_counts"] = np.stack([np.bincount(rec["idx"][:, :, l].reshape(-1), minlength=A) for l in range(L)]).astype(np.uint64)
    return dict(rec=rec, pairs=(hp.pair_counts_of(rec["idx"], ob["sites"]), np.asarray(ob["sites"], np.int32)),
                archive=har.archive_of(peeks, ob["K"]),
                stats=hs.stats_of(peeks, accepted, U, rung_hist, R, 2 * cfg["pas"] - 1))


def reference(cfg, fault=None, energy=None):
    """The CPU run of `cfg` in the layout a device run is read in (dict `run`: tr, res, peeks at the cuts, temp, anneal, recomb,
    rec, pairs, archive, stats), with its noise, the smallest margin of every kind of decision it took (`margins`) and what
    happened in it (`events`, for the coverage the CPU test asserts). `fault`: one of FAULTS[dynamics], planted in the reference."""
    dyn, n, T, L, pas, wt = cfg["dynamics"], cfg["n"], cfg["T"], cfg["L"], cfg["pas"], cfg["wt"]
    mu_max = 2 * pas - 1
    if energy is None:
        J, h, cnn = model_parts(cfg)
        energy = oracle_energy(J, h, cfg["i0"], wt, cnn, cfg["lamda"])
    noise = [orc.device_noise(cfg["seed"], cfg["chain_offset"], n, t, pas, L) for t in range(T)]
    x0 = cfg["start"].astype(np.int64)
    parts = _runner(cfg, energy, x0, noise, fault)
    cat = lambda key, axis: np.concatenate([_np(p[key]) for p in parts], axis)
    states, e_hist, f_hist = cat("states", 1), cat("energy_history", 1).astype(np.float32), cat("fitness_history", 1).astype(np.float32)
    accepted = cat("accepted", 1).astype(np.uint8)
    U = np.stack([nz[0].numpy() for nz in noise]).astype(np.int32)
    flat = np.full((T, mu_max, n), -1, np.int32)
    log_acc = np.zeros((T, n), np.float32)
    col = 0
    for p in parts:
        k = _np(p["accepted"]).shape[1]
        for t, o in enumerate(p["traces"]):
            f = _np(o["flat"])
            flat[t, :f.shape[0], col:col + k] = f
            log_acc[t, col:col + k] = _np(o["log_acc"])
        col += k
    best_idx = cat("best_idx", 0).astype(np.uint8)
    best_step = cat("best_step", 0) if "best_step" in parts[0] else e_hist.argmax(0)          # (first index on ties: the strict rule)
    # the population after t iterations as ppde_chains_peek shows it: in the default mode behind the mutation-cap reset
    dist = (states != wt[None, None]).sum(2)
    post = states.copy()
    if dyn == "default" and cfg["nmut"]:
        over = dist >= cfg["nmut"]
        over[0] = False
        post[over] = wt
    peeks = har.peeks_of(post, e_hist, f_hist, wt)
    for t in range(1, T + 1):
        peeks[t]["accepted"] = accepted[t - 1]
    peeks[0]["accepted"] = np.zeros(n, np.uint8)
    run = dict(tr=dict(flat=flat, accepted=accepted, log_acc=log_acc, U=U),
               res=dict(energy_history=e_hist, fitness_history=f_hist, best_idx=best_idx, best_step=best_step.astype(np.int32),
                        random_traj=states[:, 0].astype(np.uint8)),
               peeks=[peeks[t] for t in np.cumsum(cfg["cuts"])], temp=None, anneal=None, recomb=None)
    margins, events = {}, dict(cap_reached=bool(cfg["nmut"] and (dist >= cfg["nmut"] - 1).any()))
    pt = cfg.get("patterns")
    if pt is not None:                 # a vetoed proposal's |log_acc - log u| decides nothing: it counts as refused in the margin
        for p in parts:
            p["traces"] = [dict(o, refused=o["refused"] | o["veto"]) for o in p["traces"]]
    acc_m, gap = zip(*[hm.margins([(nz[0][sl], nz[1][:, sl], nz[2][sl]) for nz in noise], p)
                       for p, sl in zip(parts, _slices(parts))])
    margins.update(accept=min(acc_m), gap=min(gap))
    rung_hist = None
    if dyn == "tempering":
        p = parts[0]
        rung_hist = p["rung_history"]
        run["temp"] = dict(hist=p["rung_history"], rung=p["rung"], beta=p["beta"], swap_attempts=p["swap_attempts"], swap_accepts=p["swap_accepts"])
        margins["swap"] = float(p["swap_margin"])
        events["accepted_swap"] = bool(p["swap_accepts"].sum())
    if dyn in ("anneal", "adaptive"):
        D = cfg["deme"]
        parent = np.concatenate([p["parent"] + i * (D if dyn == "adaptive" else 0) for i, p in enumerate(parts)], 1).astype(np.int32)
        E = parent.shape[0]
        if dyn == "anneal":
            sched = np.asarray(cfg["schedule"], np.float32)
            before, after = (np.tile(sched[k:k + E, None], (1, n // D)) for k in (0, 1))
        else:
            path = np.stack([p["beta_path"] for p in parts], 1)
            before, after = path[:-1], path[1:]
        run["anneal"] = dict(events=E, parent=parent, pre_energy=cat("pre_energy", 1).astype(np.float32), log_mean_w=cat("log_mean_w", 1),
                             ess=cat("ess", 1), beta=cat("beta", 0), beta_before=before, beta_after=after)
        margins["select"] = min(float(p["select_margin"]) for p in parts)
        events["replaced_slot"] = bool((parent != np.arange(n)[None]).any())
    if dyn == "recombine":
        p = parts[0]
        run["recomb"] = {k: np.asarray(p[k]) for k in ("partner", "lo", "hi", "differ", "child_dist", "outcome", "log_ratio", "pre_energy",
                                                        "child_energy")}
        sites = hrc.open_list(L, cfg["min_pos"], cfg["max_pos"], cfg["library"])
        run["recomb"].update(events=p["partner"].shape[0], open_sites=sites.astype(np.int32))
        m = np.inf
        for e in range(p["partner"].shape[0]):
            a = np.minimum(np.arange(n), p["partner"][e])
            u = hrc.cut(cfg["seed"], cfg["chain_offset"] + a, (e + 1) * cfg["every"] - 1, len(sites))[2]
            free = None
            if pt is not None:
                ev = hrc.event(p["post_accept"][(e + 1) * cfg["every"] - 1][0], wt, sites, e, (e + 1) * cfg["every"] - 1, cfg["deme"],
                               cfg["seed"], cfg["chain_offset"], "round0" if fault == "round0" else None)
                free = motifs.is_free(ev["children"], pt, wt, cfg["allow_native"])
                free = free & free[p["partner"][e]]
            out, _ = hrc.outcomes(p["log_ratio"][e], u, p["child_dist"][e], p["partner"][e], p["child_energy"][e], cfg["nmut"], free)
            assert np.array_equal(out, p["outcome"][e]) or fault
            with np.errstate(over="ignore"):
                m = min(m, float(np.abs(np.exp(p["log_ratio"][e].astype(np.float64)) - u)[out < 2].min(initial=np.inf)))
        margins["cross"] = m
        events["exchange"] = bool(((p["outcome"] == 1) & (p["differ"] > 0)).any())
    if cfg["observers"] is not None:
        seen = peeks
        if fault in ("observers_before_selection", "observers_before_event"):          # the population in front of the event
            seen = har.peeks_of(np.stack([post[0]] + [_np(s) for s, _ in parts[0]["post_accept"]]),
                                np.stack([e_hist[0]] + [_np(e) for _, e in parts[0]["post_accept"]]), f_hist, wt)
        run.update(_observers(cfg, seen, accepted, U, rung_hist))
    out = dict(run=run, noise=noise, margins=margins, events=events, states=states,
               proposals=np.stack([np.concatenate([_np(p["traces"][t]["proposal"]) for p in parts], 0) for t in range(T)]))
    if dyn == "recombine":
        out["pre_event"] = [parts[0]["post_accept"][(e + 1) * cfg["every"] - 1][0] for e in range(run["recomb"]["events"])]
    if pt is not None:
        log = [p["veto_log"] for p in parts]
        veto, first, decided = (np.stack([np.concatenate([lg[t][k] for lg in log]) for t in range(T)]) for k in range(3))
        run["forbid"] = dict(n_patterns=len(pt), allow_native=cfg["allow_native"], vetoes=cat("vetoes", 0),
                             active=motifs.active_words(pt, L, wt, cfg["allow_native"]))
        out.update(veto=veto, first_pattern=first, decided=decided)
        events.update(vetoed=bool(veto.any()), accepted_move=bool((accepted.astype(bool) & (out["proposals"] != states[:-1]).any(2)).any()))
        if fault is None:              # every state the run can show is free: what the observers hold is among them
            assert motifs.is_free(states.reshape(-1, L), pt, wt, cfg["allow_native"]).all() and run["forbid"]["vetoes"].sum() == first[first >= 0].size
            assert motifs.is_free(best_idx, pt, wt, cfg["allow_native"]).all()
            if cfg["observers"] is not None:
                assert motifs.is_free(run["rec"]["idx"].reshape(-1, L), pt, wt, cfg["allow_native"]).all()
                ar = run["archive"]
                assert all(motifs.is_free(ar["idx"][b, :ar["count"][b]], pt, wt, cfg["allow_native"]).all() for b in range(n) if ar["count"][b])
                assert all(motifs.is_free(pk["idx"], pt, wt, cfg["allow_native"]).all() for pk in run["peeks"])
    return out


def _slices(parts):
    col = 0
    for p in parts:
        k = _np(p["accepted"]).shape[1]
        yield slice(col, col + k)
        col += k


def near_ties(ref):
    """The kinds of decision of a reference run that sit inside their threshold (empty: the draw is kept). A run under forbidden
    patterns that vetoed nothing or accepted no move is discarded with them."""
    idle = [k for k in ("vetoed", "accepted_move") if ref["events"].get(k) is False]
    return [k for k, v in ref["margins"].items() if not v > NEAR[k]] + idle


_KEPT = {}


def kept(seed, trials, dynamics=None, graph_len=0, forbid=False):
    """The first `trials` kept configurations of seed `seed` with their references: [(cfg, ref)], and the number of draws discarded.
    Slot i pins dynamics and library by turns, so that every combination comes up; a discarded draw is replaced by the next draw of
    the same stream for the same slot. `forbid`: configurations with forbidden patterns, allow_native by turns behind the library
    (dynamics x library x allow_native come round every 4 len(pool) slots); a draw for which no patterns could be built is
    discarded too. A pure function of its arguments (cached per process)."""
    key = (seed, trials, dynamics, graph_len) + ((True,) if forbid else ())
    if key not in _KEPT:
        rng = np.random.default_rng(seed)
        pool = (REVERSIBLE if forbid else DYNAMICS) if dynamics is None else tuple(dynamics)
        out, discarded = [], 0
        while len(out) < trials:
            i = len(out)
            if forbid:
                cfg = draw(rng, pool[i % len(pool)], (i // len(pool)) % 2, graph_len, True, (i // (2 * len(pool))) % 2 == 0)
            else:
                cfg = draw(rng, pool[i % len(pool)], (i // len(pool)) % 2, graph_len)
            ref = reference(cfg) if cfg is not None else None
            if ref is None or near_ties(ref):
                discarded += 1
                assert discarded <= 4 * trials, "the generator discards almost everything"
                continue
            out.append((cfg, ref))
        _KEPT[key] = (out, discarded)
    return _KEPT[key]


# ------------------------------------------------------------------------------------------------ the comparison
def _close(got, want, tol):
    """Worst |got - want| / (tol max(1, |want|)) over the finite entries; entries that are not finite must be equal."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return np.inf
    fin = np.isfinite(got) & np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin], equal_nan=True):
        return np.inf
    return float((np.abs(got[fin] - want[fin]) / (tol * np.maximum(1.0, np.abs(want[fin])))).max(initial=0.0))


def compare(cfg, run, ref):
    """A run in the device's layout against the reference of the same configuration: the list of what differs (empty: equal).
    Exact: path lengths, draws up to U, accept bits, the states, mutation counts and accept bits at every cut, best states and
    steps, the recorded trajectory, rung history and swap counters, parents, the recombination records, recorder rows, site and
    pair counts, the archive's contents and order, the nine statistics counters. Energies and fitness within
    helpers_modes' E_TOL / F_TOL of max(1, |value|), log_acc within LOG_ACC_TOL, adaptive betas by helpers_anneal_adaptive.check_event,
    ess and log_mean_w within 1e-12 of helpers_anneal.plan on the run's own energies."""
    exp, why = ref["run"], []
    T, n = cfg["T"], cfg["n"]

    def same(label, got, want):
        if got is None and want is None:
            return
        if got is None or want is None or not np.array_equal(np.asarray(got), np.asarray(want)):
            why.append(label)

    def close(label, got, want, tol):
        r = _close(got, want, tol)
        if not r <= 1.0:
            why.append(f"{label} ({r:.2f} of the tolerance)")

    tr, ex = run["tr"], exp["tr"]
    same("path lengths", tr["U"], ex["U"])
    first = None
    for t in range(T):
        for s in range(int(ex["U"][t].max())):
            neq = (s < ex["U"][t]) & (tr["flat"][t, s] != ex["flat"][t, s])
            if neq.any() and first is None:
                first = f"draws: first at iteration {t}, sub-step {s}, chain {int(np.flatnonzero(neq)[0])}"
        neq = tr["accepted"][t].astype(bool) != ex["accepted"][t].astype(bool)
        if neq.any() and first is None:
            b = int(np.flatnonzero(neq)[0])
            first = f"accept bits: first at iteration {t}, chain {b} (log_acc {tr['log_acc'][t, b]:.7f} against {ex['log_acc'][t, b]:.7f})"
    if first:
        why.append(first)
    la_got, la_want = np.asarray(tr["log_acc"], np.float64), np.asarray(ex["log_acc"], np.float64)
    fin = np.isfinite(la_got) & np.isfinite(la_want)
    la_err = np.abs(la_got[fin] - la_want[fin])
    if not np.array_equal(la_got[~fin], la_want[~fin], equal_nan=True) or (la_err > hm.LOG_ACC_TOL).any():
        why.append(f"log_acc (worst {la_err.max(initial=0.0):.3e})")
    res, er = run["res"], exp["res"]
    close("energy history", res["energy_history"], er["energy_history"], hm.E_TOL)
    close("fitness history", res["fitness_history"], er["fitness_history"], hm.F_TOL)
    same("best states", res["best_idx"], er["best_idx"])
    same("best steps", res["best_step"], er["best_step"])
    if er["random_traj"] is not None:
        same("recorded trajectory", res["random_traj"], er["random_traj"])
    if len(run["peeks"]) != len(exp["peeks"]):
        why.append("number of cuts")
    for i, (pk, pe) in enumerate(zip(run["peeks"], exp["peeks"])):
        for k in ("idx", "dist", "accepted"):
            same(f"cut {i}: {k}", pk[k], pe[k])
        close(f"cut {i}: energy", pk["energy"], pe["energy"], hm.E_TOL)
        close(f"cut {i}: fitness", pk["fitness"], pe["fitness"], hm.F_TOL)
    if exp["temp"] is not None:
        for k in ("hist", "rung", "beta", "swap_attempts", "swap_accepts"):
            same(f"tempering: {k}", run["temp"][k], exp["temp"][k])
    if exp["anneal"] is not None:
        an, ea, D = run["anneal"], exp["anneal"], cfg["deme"]
        same("annealing: events", an["events"], ea["events"])
        same("annealing: parents", an["parent"], ea["parent"])
        close("annealing: pre_energy", an["pre_energy"], ea["pre_energy"], hm.E_TOL)
        adaptive = cfg["dynamics"] == "adaptive"
        if not adaptive:
            for k in ("beta", "beta_before", "beta_after"):
                same(f"annealing: {k}", an[k], ea[k])
        elif an["beta_after"].shape == ea["beta_after"].shape and an["events"]:
            same("annealing: beta now", an["beta"], np.repeat(an["beta_after"][-1], D))
            same("annealing: beta path", an["beta_before"][1:], an["beta_after"][:-1])
            same("annealing: beta start", an["beta_before"][0], np.full(n // D, np.float32(cfg["beta_start"])))
        first_chain = cfg["chain_offset"] + np.arange(n // D) * D
        for e in range(min(an["events"], ea["events"])):
            us = ha.select_uniforms(cfg["seed"], first_chain, (e + 1) * cfg["every"] - 1)
            for d in range(n // D):
                sl = slice(d * D, (d + 1) * D)
                got_parent = an["parent"][e, sl] - d * D
                if adaptive:
                    fails, _, _ = haa.check_event(an["pre_energy"][e, sl], an["beta_before"][e, d], an["beta_after"][e, d], cfg["beta_end"],
                                                  cfg["ess_target"], cfg["min_step"], us[d], got_parent, an["log_mean_w"][e, d], an["ess"][e, d])
                    why += [f"annealing: event {e} deme {d}: {f}" for f in fails]
                    continue
                db = float(np.float64(an["beta_after"][e, d]) - np.float64(an["beta_before"][e, d]))
                p = ha.plan(an["pre_energy"][e, sl], db, us[d])
                if abs(an["log_mean_w"][e, d] - p["log_mean_w"]) > PLAN_REL * max(abs(p["log_mean_w"]), np.finfo(float).tiny):
                    why.append(f"annealing: event {e} deme {d}: log_mean_w {an['log_mean_w'][e, d]!r} against {p['log_mean_w']!r}")
                if abs(an["ess"][e, d] - p["ess"]) > PLAN_REL * p["ess"]:
                    why.append(f"annealing: event {e} deme {d}: ess {an['ess'][e, d]!r} against {p['ess']!r}")
    if exp["recomb"] is not None:
        rc, ec = run["recomb"], exp["recomb"]
        for k in ("events", "open_sites", "partner", "lo", "hi", "differ", "child_dist", "outcome"):
            same(f"recombination: {k}", rc[k], ec[k])
        for k in ("pre_energy", "child_energy"):
            close(f"recombination: {k}", rc[k], ec[k], hm.E_TOL)
        if np.asarray(rc["partner"]).shape == np.asarray(ec["partner"]).shape:
            ce, pe, pa = (np.asarray(rc[k]) for k in ("child_energy", "pre_energy", "partner"))
            rows = np.arange(pa.shape[0])[:, None]
            a, b = np.minimum(np.arange(n)[None], pa), np.maximum(np.arange(n)[None], pa)
            with np.errstate(invalid="ignore"):
                d32 = (ce[rows, a] - pe[rows, a]) + (ce[rows, b] - pe[rows, b])
            same("recombination: log_ratio is not the fp32 sum of its own records", rc["log_ratio"], d32.astype(np.float32))
    if cfg.get("patterns") is not None:
        fb, eb = run["forbid"], exp["forbid"]
        same("forbidden patterns: vetoes", fb["vetoes"], eb["vetoes"])
        same("forbidden patterns: n_patterns", fb["n_patterns"], len(cfg["patterns"]))
        same("forbidden patterns: allow_native", bool(fb["allow_native"]), cfg["allow_native"])
        same("forbidden patterns: active", fb["active"], motifs.active_words(cfg["patterns"], cfg["L"], cfg["wt"], cfg["allow_native"]))
    if cfg["observers"] is not None:
        rec, erec = run["rec"], exp["rec"]
        for k in ("rows", "chain", "idx", "site_counts"):
            same(f"recorder: {k}", rec[k], erec[k])
        close("recorder: energy", rec["energy"], erec["energy"], hm.E_TOL)
        close("recorder: fitness", rec["fitness"], erec["fitness"], hm.F_TOL)
        same("pair counts", run["pairs"][0], exp["pairs"][0])
        same("pair sites", run["pairs"][1], exp["pairs"][1])
        for k in ("idx", "step", "count"):
            same(f"archive: {k}", run["archive"][k], exp["archive"][k])
        close("archive: energy", run["archive"]["energy"], exp["archive"]["energy"], hm.E_TOL)
        close("archive: fitness", run["archive"]["fitness"], exp["archive"]["fitness"], hm.F_TOL)
        for k in hs.KEYS:
            same(f"statistics: {k}", run["stats"][k], exp["stats"][k])
    return why


# ------------------------------------------------------------------------------------------------ what a pattern run showed
def veto_facts(cfg, ref):
    """What the vetoes of a kept configuration's reference run fell on: {item of tests/test_fuzz_modes_cpu.py's list: bool}. Every
    position and match count is motifs.find / motifs.matches on the run's own proposals."""
    pt, wt, L, T, n = cfg["patterns"], cfg["wt"], cfg["L"], cfg["T"], cfg["n"]
    native, lib = cfg["allow_native"], cfg["library"]
    veto, acc, props = ref["veto"], ref["run"]["tr"]["accepted"].astype(bool), ref["proposals"]
    act = motifs.active_mask(pt, L, wt, native)
    wt_hits = motifs.matches(np.asarray(wt)[None], pt)[0]                  # [M, L]
    frozen = np.ones(L, bool)
    frozen[cfg["min_pos"]:cfg["max_pos"] + 1] = False
    if lib is not None:
        frozen |= np.asarray(lib) == 0
    f = dict.fromkeys(("start >= 64", "window across lanes 63 | 64", "last start", "context", "two patterns", "native elsewhere"), False)
    for t, b in zip(*np.nonzero(veto)):
        m, p = (int(v[0]) for v in motifs.find(props[t, b][None], pt, wt, native))
        k = int(pt.lengths[m])
        assert m >= 0 and m == ref["first_pattern"][t, b]
        f["start >= 64"] |= p >= 64
        f["window across lanes 63 | 64"] |= p < 64 <= p + k - 1
        f["last start"] |= p == L - k
        f["context"] |= bool(frozen[p:p + k].any())
        f["two patterns"] |= int((motifs.matches(props[t, b][None], pt)[0] & act).any(1).sum()) >= 2
        f["native elsewhere"] |= bool(native and wt_hits[m].any())
    f["decided by the veto alone"] = bool(ref["decided"].any())
    f["veto behind an accepted proposal"] = bool((veto[1:] & acc[:-1]).any())
    f["accepted behind a veto"] = bool((acc[1:] & veto[:-1]).any())
    f["outcome 4"] = cfg["dynamics"] == "recombine" and bool((ref["run"]["recomb"]["outcome"] == 4).any())
    f["veto behind a replaced slot"] = False
    if cfg["dynamics"] in ("anneal", "adaptive"):
        par = ref["run"]["anneal"]["parent"]
        f["veto behind a replaced slot"] = any(bool((veto[(e + 1) * cfg["every"]] & (par[e] != np.arange(n))).any())
                                               for e in range(par.shape[0]) if (e + 1) * cfg["every"] < T)
    f["veto behind a swap"] = False
    if cfg["dynamics"] == "tempering":
        h = ref["run"]["temp"]["hist"]
        f["veto behind a swap"] = bool((veto[1:] & (h[1:T] != h[:T - 1])).any())
    return f

"""The runs behind tests/golden/chain_bits_parent.npz: small device-RNG chains on seeded synthetic Potts models whose every
recorded bit -- path lengths, moves, accept bits, log_acc, histories, best and final states -- pins the chain kernels
(ppde_amd/csrc/pas.h). scripts/record_chain_bits.py writes the fixture from a library build, tests/test_chain_path_gpu.py
replays the same runs on the built library and compares integer views."""
import numpy as np
import torch

from ppde_amd import library as dl, synthetic
from ppde_amd.energy import HipModel
from ppde_amd.sampler import Chains

FIXTURE = "chain_bits_parent.npz"
TRACED = ("U", "flat", "accepted", "log_acc")
COLLECTED = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_step")


def _model(L, Lp, i0, seed, h_plus=()):
    """(HipModel, wild type uint8 [L], J, h) of a seeded Potts window [i0, i0 + Lp) in a seeded sequence of L."""
    wt = np.random.default_rng(1000 + seed).integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed)
    h = h.copy()
    for l, k, v in h_plus:
        h[l, k] += np.float32(v)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    m.set_lamda(0.0)
    return m, wt, J, h


def _policies(stem, **kw):
    return {f"{stem}_{'reuse' if r else 'reeval'}": dict(kw, reuse=r) for r in (False, True)}


def cases():
    """name -> run description. Every run: `which` 1 (Potts product of experts), device RNG, wild-type start."""
    c = {}
    # a: one residue group per thread, a short sequence; pas_length 5 gives paths of up to 9 moves (the variate refill every
    #    PAS_QS sub-steps, three-row reverse passes followed by shorter ones), nmut_threshold 3 the flip of the cap's mask
    for pas in (1, 2, 5):
        for nmut in (0, 3):
            c.update(_policies(f"a_pas{pas}_nmut{nmut}", L=24, Lp=20, i0=2, seed=11, n=5, T=16, pas=pas, nmut=nmut))
    #    ... and pas_length 40 paths of more than 64 moves: more sub-steps than wave 0, which writes the path's records, has lanes
    c.update(_policies("a_pas40_nmut0", L=24, Lp=20, i0=2, seed=11, n=4, T=6, pas=40, nmut=0, longest=65))
    # b: the benchmark's geometry: with trace buffers the general kernels, without them the pinned instantiations
    c.update(_policies("b_traced", L=96, Lp=80, i0=8, seed=12, n=8, T=12, pas=2, nmut=0))
    c.update(_policies("b_untraced", L=96, Lp=80, i0=8, seed=12, n=8, T=12, pas=2, nmut=0, trace=False))
    # c, d, e: lane + 64 r < L at its edge; two and three residue groups per thread (four and five residues per lane)
    c.update(_policies("c_L65", L=65, Lp=60, i0=3, seed=13, n=4, T=8, pas=2, nmut=0))
    c.update(_policies("d_L104", L=104, Lp=90, i0=7, seed=14, n=4, T=8, pas=2, nmut=0))
    c.update(_policies("e_L237", L=237, Lp=120, i0=50, seed=15, n=3, T=6, pas=2, nmut=0))
    # f: the LIB / REV / TEMP instantiations of the same bodies
    c.update(_policies("f_library", L=24, Lp=20, i0=2, seed=16, n=6, T=12, pas=2, nmut=0, mode="library"))
    c.update(_policies("f_reversible", L=24, Lp=20, i0=2, seed=16, n=6, T=12, pas=2, nmut=3, mode="reversible"))
    c.update(_policies("f_tempering", L=24, Lp=20, i0=2, seed=16, n=6, T=12, pas=2, nmut=3, mode="tempering"))
    return c


def case_library(wt, lo, hi):
    """A design library over [lo, hi]: two letters dropped everywhere, every fifth residue frozen."""
    words = dl.build_library(wt, window=(lo, hi), exclude="CW")
    words[lo + 2:hi + 1:5] = 0
    return dl.fold_range(words, lo, hi)


def run_case(spec, use_graph=True):
    """One run of `cases()`: dict of arrays (the TRACED ones only with trace buffers), plus the final states."""
    spec = dict(spec)
    spec.pop("longest", None)                         # (what the fixture's own check asks of the longest path drawn)
    mode, trace = spec.get("mode"), spec.get("trace", True)
    m, wt, _, _ = _model(spec["L"], spec["Lp"], spec["i0"], spec["seed"])
    lo, hi = spec["i0"], spec["i0"] + spec["Lp"] - 1
    lib = mode is not None
    ch = Chains(m, spec["n"], spec["T"], spec["pas"], spec["nmut"], False, 0 if lib else lo, spec["L"] - 1 if lib else hi, 1, 1,
                reuse_grad=spec["reuse"], trace=trace, random_chain=1, use_graph=use_graph, seed=7000 + spec["seed"])
    if mode == "library":
        ch.set_library(case_library(wt, lo, hi))
    elif mode in ("reversible", "tempering"):
        ch.set_library(dl.fold_range(dl.full_library(spec["L"]), lo, hi))
        ch.set_reversible(True)
        if mode == "tempering":
            ch.set_tempering([1.0, 0.5], 2)
    ch.init(torch.as_tensor(np.tile(wt, (spec["n"], 1))).cuda())
    ch.run(spec["T"])
    ch.sync()
    out = {}
    if trace:
        tr = ch.trace()
        out.update({k: tr[k] for k in TRACED})
    res = ch.collect()
    out.update({k: res[k] for k in COLLECTED})
    out["random_traj"] = res["random_traj"]
    out["final_idx"] = ch.peek()["idx"]
    if mode == "tempering":
        out["rung_history"] = ch.tempering_history()
    ch.close()
    return out


def bits(a):
    """Integer view of an array: floats compare by their bits (NaN included), integers as they are."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def record(names=None, use_graph=True):
    """{'<case>/<field>': array} of the named cases (default: all)."""
    cs = cases()
    out = {}
    for name in (names or cs):
        for k, v in run_case(cs[name], use_graph).items():
            out[f"{name}/{k}"] = v
    return out


def two_dominant_sites_model(L=96, Lp=80, sites=(3, 40), boost=30.0, seed=17):
    """A Potts window [0, Lp) with a field of +boost on one non-wild-type letter of each of `sites`: thread t of the chain
    kernels' 512 holds letters 4t .. 4t + 3, so residue l sits in wave (5 l) // 64 -- residues 3 and 40 in waves 0 and 3."""
    wt = np.random.default_rng(1000 + seed).integers(0, 20, L).astype(np.uint8)
    plus = [(l, (int(wt[l]) + 7) % 20, boost) for l in sites]
    m, wt, J, h = _model(L, Lp, 0, seed, plus)
    return m, wt, J, h, plus

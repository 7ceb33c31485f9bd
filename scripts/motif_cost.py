#!/usr/bin/env python3
"""What forbidden patterns cost a reversible run, and that the run without the mode costs what it did: BASELINE
config 2's geometry -- PABP, Potts-only product of experts, 128 chains, device RNG, hipGraph replay, no trace -- as a reversible
run (a library of all letters over the Potts window, range folded in, as PPDE_PAS runs such chains), from one process tree and
under both evaluation policies:

  off          the reversible run without the mode
  on           the same run with 32 patterns of length 8 set (the most the veto kernel ever scans: 32 bits in every active word)
  parent       the reversible run on the parent commit's library, in the same call (a difference beyond the call's own
               run-to-run spread is a regression of the default path)

  python scripts/motif_cost.py --parent-lib <parent checkout>/ppde_amd/libppde_hip.so [--steps 2000] [--out profiles/motif_cost.md]

Every run is a fresh child process (`--child`), each under its own time limit; the tree stops at the first child that fails.
`off` is run twice: the difference of its two figures is the spread the others are read against."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TAG = "[motif_cost] "


def patterns():
    """32 patterns of length 8 that veto little, so the run stays the run: every element is a random set of six letters. The veto
    kernel tests all eight elements of every active (pattern, start) whatever they hold, so its work is that of any such set."""
    import numpy as np
    from ppde_amd import motifs
    rng = np.random.default_rng(7)
    el = np.zeros((32, 8), np.uint32)
    for m in range(32):
        for j in range(8):
            el[m, j] = sum(1 << int(k) for k in rng.choice(20, size=6, replace=False))
    return motifs.Patterns(el, [8] * 32)


def child(a):
    import numpy as np
    import torch
    from ppde_amd import _hip, library, synthetic
    if a.variant == "parent":                       # (the parent's library does not export the mode's entry points)
        for name in [k for k in _hip.SIGNATURES if "forbidden" in k or "motif" in k]:
            _hip.SIGNATURES.pop(name)
    from ppde_amd.encoding import seqs_to_idx
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    _, seq, (i0, Lp) = synthetic.PROTEINS["PABP_YEAST_Fields2013"]
    wt = seqs_to_idx([seq])[0]
    L = len(wt)
    J, h = synthetic.make_potts(Lp, seed=1234)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    T = a.warmup + a.steps
    ch = Chains(m, a.chains, T, 2, 0, False, 0, L - 1, 1, 1, reuse_grad=bool(a.reuse), random_chain=-1, seed=1, use_graph=True)
    ch.set_library(library.fold_range(library.full_library(L), i0, i0 + Lp - 1))
    ch.set_reversible(True)
    if a.variant == "on":
        ch.set_forbidden(patterns())
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    e = ch.collect()["energy_history"]
    rec = {"variant": a.variant, "reuse": a.reuse, "steps_per_s": a.steps / dt, "us_per_step": dt / a.steps * 1e6,
           "energy_sum": float(e.astype(np.float64).sum()), "replayed": ch.graph_stats()["replayed_steps"]}
    if a.variant == "on":
        from ppde_amd import motifs
        rec["vetoed"] = motifs.summarise(ch.forbidden_state()["vetoes"], T)["share"]
    print(TAG + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variant", default="off")
    ap.add_argument("--reuse", type=int, default=0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--parent-lib", default=None, help="libppde_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motif_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = ["off"] + (["parent"] if a.parent_lib else []) + ["on", "off"] + (["parent"] if a.parent_lib else []) + ["on"]
    lines = ["# Cost of forbidden patterns in a reversible run (scripts/motif_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, reversible mode over a library of all letters in the Potts",
             f"window, {a.steps} timed iterations behind {a.warmup} of warm-up, one fresh process per row. `off`: without the mode (twice:",
             "the difference is the call's own run-to-run spread); `parent`: the same run on the parent commit's library; `on`: 32",
             "patterns of length 8 set (one veto launch per iteration). `on - off`: the mean of the `on` rows minus the mean of the `off` rows.", ""]
    if not a.parent_lib:
        lines += ["No `--parent-lib` was given: the parent commit's rows are missing.", ""]
    lines += ["| policy | run | us / step | steps/s | replayed | proposals vetoed |", "|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        recs = []
        for v in variants:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            env = dict(os.environ, PPDE_HIP_LIB=os.path.abspath(a.parent_lib)) if v == "parent" else dict(os.environ)
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            got = [l for l in r.stdout.splitlines() if l.startswith(TAG)]
            if r.returncode != 0 or not got:
                sys.exit(f"{v} (reuse {reuse}): status {r.returncode}; stopping here\n" + r.stdout[-2000:] + r.stderr[-3000:])
            recs.append(json.loads(got[-1][len(TAG):]))
        off = [r_["us_per_step"] for r_ in recs if r_["variant"] == "off"]
        on = [r_["us_per_step"] for r_ in recs if r_["variant"] == "on"]
        base, spread = sum(off) / len(off), max(off) - min(off)
        policy = "reuse" if reuse else "re-evaluate"
        for r_ in recs:
            vet = f"{r_['vetoed']:.3f}" if "vetoed" in r_ else ""
            lines.append(f"| {policy} | {r_['variant']} | {r_['us_per_step']:.3f} | {r_['steps_per_s']:.0f} | {r_['replayed']} | {vet} |")
        lines.append(f"| {policy} | spread of `off` | {spread:.3f} | | | |")
        lines.append(f"| {policy} | on - off | {sum(on) / len(on) - base:+.3f} ({(sum(on) / len(on) - base) / base * 100:+.1f} % of an iteration) | | | |")
        par = [r_ for r_ in recs if r_["variant"] == "parent"]
        if par:
            off_recs = [r_ for r_ in recs if r_["variant"] == "off"]
            assert all(p["energy_sum"] == off_recs[0]["energy_sum"] for p in par), "the run without the mode must compute what the parent commit computed"
            pm = sum(p["us_per_step"] for p in par) / len(par)
            lines.append(f"| {policy} | off - parent | {base - pm:+.3f} | | | |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

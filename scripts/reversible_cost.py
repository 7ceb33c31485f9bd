#!/usr/bin/env python3
"""What reversible mode costs the chain kernels, and that the default path costs what it did: BASELINE config
2's geometry -- PABP, Potts-only product of experts, 128 chains, device RNG, hipGraph replay, no trace -- three ways from one
process tree and under both evaluation policies:

  reversible   a library of all letters over the Potts window (range folded in, as PPDE_PAS runs such chains) + set_reversible:
               `k_accept_rev` / `k_accept_propose_rev`, general instantiations
  default      the same run without set_reversible: `k_accept` / `k_accept_propose_lib` of the SAME build (the per-launch comparison)
  parent       config 2 itself (no library) on this build AND on the parent commit's library, in the same call: the default
               path's steps/s before and after (a difference beyond the +-3 % box-to-box spread of DESIGN.md §9 is a regression)

  python scripts/reversible_cost.py --parent-lib <parent checkout>/ppde_amd/libppde_hip.so [--steps 2000] [--out profiles/reversible_cost.md]

(`git worktree add ../parent HEAD~1 && (cd ../parent && python -m ppde_amd.build)` makes that library; without --parent-lib the
parent rows are left out and the file says so.) For each run a fresh child process is started twice: once plainly, timing
`--steps` iterations (steps/s), and once under `rocprofv3 --kernel-trace --stats` (no counters), from whose per-kernel table
the chain kernels' average durations are read. `--child` is that child."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def child(a):
    import numpy as np
    import torch
    from ppde_amd import _hip, library, synthetic
    if a.variant == "parent":                       # (the parent's library does not export the mode's entry point)
        _hip.SIGNATURES.pop("ppde_chains_set_reversible", None)
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
    with_lib = a.variant in ("reversible", "default")
    lo, hi = (0, L - 1) if with_lib else (i0, i0 + Lp - 1)
    ch = Chains(m, a.chains, T, 2, 0, False, lo, hi, 1, 1, reuse_grad=bool(a.reuse), random_chain=-1, seed=1, use_graph=True)
    if with_lib:
        ch.set_library(library.fold_range(library.full_library(L), i0, i0 + Lp - 1))
    if a.variant == "reversible":
        ch.set_reversible(True)
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    e = ch.collect()["energy_history"]
    print("[reversible_cost] " + json.dumps({"variant": a.variant, "reuse": a.reuse, "steps_per_s": a.steps / dt,
                                            "energy_sum": float(e.astype(np.float64).sum())}), flush=True)


def chain_kernel_us(stats_dir):
    f = max(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    out = {}
    for row in csv.DictReader(open(f)):
        name = row["Name"].replace("void ", "").split("(")[0]
        if name.startswith(("k_propose", "k_accept")):
            out[name] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variant", default="default", choices=["reversible", "default", "config2", "parent"])
    ap.add_argument("--reuse", type=int, default=0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--parent-lib", default=None, help="libppde_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reversible_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = ["reversible", "default", "config2"] + (["parent"] if a.parent_lib else [])
    lines = ["# Cost of reversible mode in the chain kernels (scripts/reversible_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, {a.steps} timed iterations. `reversible` / `default`: a library of",
             "all letters over the Potts window, with and without `set_reversible`, same build; `config2` / `parent`: no library, this build",
             "and the parent commit's library in the same call. steps/s from a plain run; microseconds per launch from a separate",
             "`rocprofv3 --kernel-trace --stats` run of the same command (no counters).", ""]
    if not a.parent_lib:
        lines += ["No `--parent-lib` was given: the parent commit's rows are missing.", ""]
    lines += ["| policy | run | steps/s | kernel | avg us | launches |", "|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        sums = {}
        for v in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            env = dict(os.environ, PPDE_HIP_LIB=os.path.abspath(a.parent_lib)) if v == "parent" else dict(os.environ)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:
                sys.exit(r.stdout[-2000:] + r.stderr[-3000:])
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("[reversible_cost] ")][-1][len("[reversible_cost] "):])
            sums[v] = rec["energy_sum"]
            with tempfile.TemporaryDirectory() as d:
                p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd],
                                   capture_output=True, text=True, timeout=900, env=env)
                if p.returncode != 0:
                    sys.exit(p.stdout[-2000:] + p.stderr[-3000:])
                ks = chain_kernel_us(d)
            policy = "reuse" if reuse else "re-evaluate"
            for k, (us, calls) in sorted(ks.items()):
                lines.append(f"| {policy} | {v} | {rec['steps_per_s']:.0f} | `{k}` | {us:.2f} | {calls} |")
        if "parent" in sums:
            assert sums["parent"] == sums["config2"], "the default path must compute what the parent commit computed"
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a design library costs the chain kernels: BASELINE config 2's geometry -- PABP, Potts-only product of
experts, 128 chains, device RNG, hipGraph replay, no trace, proposals over the Potts window -- with a library of ALL TWENTY
LETTERS AT EVERY RESIDUE (the library's words are read and applied but nothing is forbidden, so by the feature's contract the
trajectory is the one of the run without a library, bit for bit; the position range stays the window in both runs, with its
2^-23 floor entries) against the same run without a library, under both evaluation policies.

  python scripts/library_cost.py [--steps 2000] [--out profiles/library_cost.md]

For each of the four runs a fresh child process is started twice: once plainly, timing `--steps` iterations (steps/s), and once
under `rocprofv3 --kernel-trace --stats` (no counters), from whose per-kernel table the chain kernels' average durations are
read. `--child` is that child."""
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
    from ppde_amd import library, synthetic
    from ppde_amd.encoding import seqs_to_idx
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    _, seq, (i0, Lp) = synthetic.PROTEINS["PABP_YEAST_Fields2013"]
    wt = seqs_to_idx([seq])[0]
    J, h = synthetic.make_potts(Lp, seed=1234)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    T = a.warmup + a.steps
    ch = Chains(m, a.chains, T, 2, 0, False, i0, i0 + Lp - 1, 1, 1, reuse_grad=bool(a.reuse), random_chain=-1, seed=1, use_graph=True)
    if a.library:
        ch.set_library(library.full_library(len(wt)))
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    e = ch.collect()["energy_history"]
    print("[library_cost] " + json.dumps({"library": a.library, "reuse": a.reuse, "steps_per_s": a.steps / dt,
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
    ap.add_argument("--library", type=int, default=0)
    ap.add_argument("--reuse", type=int, default=0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "library_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = ["# Cost of a design library in the chain kernels (scripts/library_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, {a.steps} timed iterations; a library of all letters at",
             "every residue against no library (same position range, same trajectory bit for bit). steps/s from a plain run; microseconds per launch from a separate",
             "`rocprofv3 --kernel-trace --stats` run of the same command (no counters).", "",
             "| policy | library | steps/s | kernel | avg us | launches |", "|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        sums = []
        for lib in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--library", str(lib), "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stdout[-2000:] + r.stderr[-3000:])
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("[library_cost] ")][-1][len("[library_cost] "):])
            sums.append(rec["energy_sum"])
            with tempfile.TemporaryDirectory() as d:
                p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd],
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(p.stdout[-2000:] + p.stderr[-3000:])
                ks = chain_kernel_us(d)
            policy = "reuse" if reuse else "re-evaluate"
            for k, (us, calls) in sorted(ks.items()):
                lines.append(f"| {policy} | {'all letters' if lib else 'none'} | {rec['steps_per_s']:.0f} | `{k}` | {us:.2f} | {calls} |")
        assert sums[0] == sums[1], "an all-letters library must not change the trajectory"
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

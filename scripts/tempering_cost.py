#!/usr/bin/env python3
"""What parallel tempering costs a reversible run: BASELINE config 2's geometry -- PABP, Potts-only product of
experts, 128 chains, device RNG, hipGraph replay, no trace -- as a reversible run with and without a 4-rung ladder, under both
evaluation policies, from one process tree:

  reversible   a library of all letters over the Potts window (range folded in, as PPDE_PAS runs such chains) + set_reversible:
               `k_propose_lib`, `k_accept_rev` / the fused `k_accept_propose_rev`
  tempering    the same + set_tempering((1, 0.7, 0.5, 0.35), swap_every 1): `k_propose_temp`, `k_accept_temp`, `k_swap`, never
               fused (the next proposal must see the post-swap beta, the swap the post-accept energy)

  python scripts/tempering_cost.py [--steps 2000] [--out profiles/tempering_cost.md]

For each run a fresh child process is started twice: once plainly, timing `--steps` iterations (steps/s), and once under
`rocprofv3 --kernel-trace --stats` (no counters), from whose per-kernel table the average durations of the chain kernels and of
`k_swap` are read. `--child` is that child."""
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
BETAS = (1.0, 0.7, 0.5, 0.35)


def child(a):
    import numpy as np
    import torch
    from ppde_amd import library, synthetic
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
    if a.variant == "tempering":
        ch.set_tempering(BETAS, 1)
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    rec = {"variant": a.variant, "reuse": a.reuse, "steps_per_s": a.steps / dt}
    if a.variant == "tempering":
        st = ch.tempering_state()
        rec["swaps"] = [int(st["swap_accepts"].sum()), int(st["swap_attempts"].sum())]
    print("[tempering_cost] " + json.dumps(rec), flush=True)


def kernel_us(stats_dir):
    f = max(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    out = {}
    for row in csv.DictReader(open(f)):
        name = row["Name"].replace("void ", "").split("(")[0]
        if name.startswith(("k_propose", "k_accept", "k_swap")):
            out[name] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variant", default="reversible", choices=["reversible", "tempering"])
    ap.add_argument("--reuse", type=int, default=0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tempering_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = ["# Cost of parallel tempering in a reversible run (scripts/tempering_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, {a.steps} timed iterations, a library of all letters over the",
             f"Potts window. `reversible`: set_reversible alone; `tempering`: the same with the ladder {BETAS}, a swap event behind every",
             "iteration. steps/s from a plain run; microseconds per launch from a separate `rocprofv3 --kernel-trace --stats` run of the",
             "same command (no counters).", "",
             "| policy | run | steps/s | swaps accepted / attempted | kernel | avg us | launches |", "|---|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        for v in ("reversible", "tempering"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stdout[-2000:] + r.stderr[-3000:])
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("[tempering_cost] ")][-1][len("[tempering_cost] "):])
            with tempfile.TemporaryDirectory() as d:
                p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd],
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(p.stdout[-2000:] + p.stderr[-3000:])
                ks = kernel_us(d)
            policy = "reuse" if reuse else "re-evaluate"
            swaps = "{} / {}".format(*rec["swaps"]) if "swaps" in rec else "-"
            for k, (us, calls) in sorted(ks.items()):
                lines.append(f"| {policy} | {v} | {rec['steps_per_s']:.0f} | {swaps} | `{k}` | {us:.2f} | {calls} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

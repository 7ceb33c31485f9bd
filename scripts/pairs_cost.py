#!/usr/bin/env python3
"""What the pair counts cost a run: BASELINE config 2's geometry -- PABP, Potts-only product of experts, 128
chains, device RNG, hipGraph replay, no trace -- under both evaluation policies, from one process tree:

  parent          no recorder, the PARENT commit's tree and library (--parent-tree: a checkout of the parent commit with its
                  library built; left out of the table, and said so, when the flag is not given)
  none            no recorder, this build: must enqueue what the parent enqueues
  counts1         counts-only recorder, every = 1
  counts1+pairs   the same with pair counts over all residues: `k_record_pairs` behind every iteration, all of them counting
  counts10        counts-only recorder, every = 10
  counts10+pairs  the same with pair counts over all residues: one launch in ten counts (the others leave at once)

  python scripts/pairs_cost.py [--steps 2000] [--parent-tree DIR] [--out profiles/pairs_cost.md]

For each run a fresh child process is started: once plainly, timing `--steps` iterations (steps/s), and, for the runs with pair
counts, once more under `rocprofv3 --kernel-trace --stats` (no counters), from whose per-kernel table the average duration of
`k_record_pairs` is read. Two ratios are reported: pair counts against the same build's recorder-only run, and this build's
recorder-less run against the parent commit's. `--child` is that child; `--tree` is the tree it imports ppde_amd from."""
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
VARIANTS = ("parent", "none", "counts1", "counts1+pairs", "counts10", "counts10+pairs")
TAG = "[pairs_cost] "


def child(a):
    sys.path.insert(0, a.tree or REPO)
    import numpy as np
    import torch
    from ppde_amd import synthetic
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
    if a.variant.startswith("counts"):
        ch.set_recorder(10 if a.variant.startswith("counts10") else 1, keep_samples=False)
    if a.variant.endswith("+pairs"):
        ch.set_pair_counts()
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    rec = {"variant": a.variant, "reuse": a.reuse, "steps_per_s": a.steps / dt, "sites": len(seq)}
    if a.variant.startswith("counts"):
        rec["rows"] = ch.recorded()["rows"]
    if a.variant.endswith("+pairs"):
        counts, _ = ch.pair_counts()
        rec["nonzero_bins"] = int(np.count_nonzero(counts))
    print(TAG + json.dumps(rec), flush=True)


def kernel_us(stats_dir):
    found = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None, None
    f = max(found, key=os.path.getmtime)
    for row in csv.DictReader(open(f)):
        if row["Name"].replace("void ", "").split("(")[0] == "k_record_pairs":
            return float(row["AverageNs"]) / 1e3, int(row["Calls"])
    return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--variant", default="none", choices=VARIANTS)
    ap.add_argument("--reuse", type=int, default=0)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pairs_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    parent = "its tree was given with --parent-tree" if a.parent_tree else "NOT MEASURED: no --parent-tree was given"
    lines = ["# Cost of the pair counts (scripts/pairs_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, {a.steps} timed iterations, counts-only recorders, pair",
             f"counts over all residues. `parent`: the parent commit ({parent}); `none`: this build without a recorder. steps/s from a",
             "plain run; microseconds per `k_record_pairs` launch (counting or not) from a separate `rocprofv3 --kernel-trace --stats`",
             "run of the same command (no counters). `vs recorder`: steps/s over the same build's recorder-only run with the same",
             "`every`; `vs parent`: the recorder-less run of this build over the parent commit's.", "",
             "| policy | run | steps/s | vs recorder | vs parent | rows | nonzero bins | k_record_pairs avg us | launches |",
             "|---|---|---|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        sps = {}
        for v in VARIANTS:
            if v == "parent" and not a.parent_tree:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            if v == "parent":
                cmd += ["--tree", os.path.abspath(a.parent_tree)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stdout[-2000:] + r.stderr[-3000:])
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith(TAG)][-1][len(TAG):])
            us = calls = None
            if v.endswith("+pairs"):
                with tempfile.TemporaryDirectory() as d:
                    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd],
                                       capture_output=True, text=True, timeout=900)
                    if p.returncode != 0:
                        sys.exit(p.stdout[-2000:] + p.stderr[-3000:])
                    us, calls = kernel_us(d)
            sps[v] = rec["steps_per_s"]
            vs_rec = f"{sps[v] / sps[v[:-len('+pairs')]]:.3f}" if v.endswith("+pairs") else "-"
            vs_parent = f"{sps[v] / sps['parent']:.3f}" if v == "none" and "parent" in sps else "-"
            policy = "reuse" if reuse else "re-evaluate"
            lines.append(f"| {policy} | {v} | {sps[v]:.0f} | {vs_rec} | {vs_parent} | {rec.get('rows', '-')} | {rec.get('nonzero_bins', '-')} | "
                         f"{'-' if us is None else format(us, '.2f')} | {'-' if calls is None else calls} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

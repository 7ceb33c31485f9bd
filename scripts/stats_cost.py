#!/usr/bin/env python3
"""What the move statistics cost a run: BASELINE config 2's geometry -- PABP, Potts-only product of experts,
128 chains, device RNG, hipGraph replay, no trace -- under both evaluation policies, from one process tree:

  parent       no statistics, the PARENT commit's tree and library (--parent-tree: a checkout of the parent commit with its library
               built; left out of the table, and said so, when the flag is not given). Run twice, first and last, so the
               run-to-run spread is on the page
  none         no statistics, this build: must enqueue what the parent enqueues
  nosites      set_stats(per_site=False): k_stats behind every iteration, without its per-site workgroups
  sites        set_stats(per_site=True): k_stats behind every iteration

  python scripts/stats_cost.py [--steps 2000] [--parent-tree DIR] [--out profiles/stats_cost.md]

Steps/s come from plain runs, one fresh child process each, alternated within this one call (parent, none, nosites, sites, parent).
Microseconds per `k_stats` come from a `rocprofv3 --kernel-trace --stats` run of its own (no counters) of the two children. `--child`
is that child; `--tree` is the tree it imports ppde_amd from."""
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
VARIANTS = ("parent", "none", "nosites", "sites")
TAG = "[stats_cost] "


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
    if a.variant in ("nosites", "sites"):
        ch.set_stats(a.variant == "sites")
    ch.init(torch.as_tensor(np.tile(wt, (a.chains, 1))).cuda())
    ch.run(a.warmup)
    ch.sync()
    t0 = time.perf_counter()
    ch.run(a.steps)
    ch.sync()
    dt = time.perf_counter() - t0
    rec = {"variant": a.variant, "reuse": a.reuse, "steps_per_s": a.steps / dt}
    if a.variant in ("nosites", "sites"):
        st = ch.stats()
        assert int(st["iters"].sum()) == a.chains * T
        rec["acceptance"] = float(st["accepts"].sum() / st["iters"].sum())
    print(TAG + json.dumps(rec), flush=True)


def kernel_us(stats_dir):
    f = max(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    out = {}
    for row in csv.DictReader(open(f)):
        name = row["Name"].replace("void ", "").split("(")[0]
        if name == "k_stats":
            out[name] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
    return out


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stats_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    parent = "its tree was given with --parent-tree" if a.parent_tree else "NOT MEASURED: no --parent-tree was given"
    lines = ["# Cost of the move statistics (scripts/stats_cost.py)", "",
             f"PABP, Potts only, {a.chains} chains, device RNG, hipGraph replay, {a.steps} timed iterations. `parent`: the parent commit",
             f"({parent}), run first and last: the two rows are the run-to-run spread; `none`: this build without statistics;",
             "`nosites`: set_stats(per_site=False); `sites`: set_stats(per_site=True); one more launch per iteration either way. steps/s from",
             "plain runs, one fresh process each, in the order of the table; microseconds per launch from a separate `rocprofv3",
             "--kernel-trace --stats` run of the same command (no counters). ratio = steps/s over the first parent run's (over `none`",
             "where the parent was not measured); us/iteration = 1e6 / steps/s minus the same of `none`: what the statistics add to an",
             "iteration, launch boundaries included.", "",
             "| policy | run | steps/s | ratio | added us/iteration | acceptance | k_stats avg us | launches |",
             "|---|---|---|---|---|---|---|---|"]
    for reuse in (0, 1):
        base = none = None
        order = VARIANTS + ("parent",) if a.parent_tree else VARIANTS[1:]
        for v in order:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--reuse", str(reuse),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--chains", str(a.chains)]
            if v == "parent":
                cmd += ["--tree", os.path.abspath(a.parent_tree)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(r.stdout[-2000:] + r.stderr[-3000:])
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith(TAG)][-1][len(TAG):])
            us = {}
            if v in ("nosites", "sites"):
                with tempfile.TemporaryDirectory() as d:
                    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd],
                                       capture_output=True, text=True, timeout=900)
                    if p.returncode != 0:
                        sys.exit(p.stdout[-2000:] + p.stderr[-3000:])
                    us = kernel_us(d)
            base = rec["steps_per_s"] if base is None else base
            if v == "none":
                none = rec["steps_per_s"]
            added = "-" if v in ("parent", "none") or none is None else format(1e6 / rec["steps_per_s"] - 1e6 / none, ".2f")
            policy = "reuse" if reuse else "re-evaluate"
            c_us = us.get("k_stats")
            acc = format(rec["acceptance"], ".3f") if "acceptance" in rec else "-"
            lines.append(f"| {policy} | {v} | {rec['steps_per_s']:.0f} | {rec['steps_per_s'] / base:.3f} | {added} | {acc} | "
                         f"{'-' if c_us is None else format(c_us[0], '.2f')} | "
                         f"{'-' if c_us is None else c_us[1]} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

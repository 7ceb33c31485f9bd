#!/usr/bin/env python3
"""A/B of two library builds on config 2 as bench.py builds it (PABP Potts product of experts, 128 chains, device RNG, hipGraph
replay): each library runs in its own fresh child process (PPDE_HIP_LIB), in the order A, B, A, B, each child under its own
`timeout -k 10`; the chain stops at the first non-zero status. Per child and evaluation policy: the median us per step over 5
blocks of 2000 steps and over 50 blocks of 20 steps, and a checksum of the energy history (equal bits on both sides).

    python scripts/ab_chain.py lib_a.so lib_b.so [--limit 240]

The verdict printed at the end is on the re-evaluating policy's long-block figure: `spread` is the largest difference between
the two runs of one library, B's gain over A counts when B is faster in both pairings and its median gain is >= 3 x spread.
"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, time, json
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import ctypes
from ppde_amd import _hip
_old = ctypes.CDLL(_hip.LIB_PATH)                  # an older build lacks the entry points added since; nothing here calls them
for _name in [k for k in _hip.SIGNATURES if not hasattr(_old, k)]:
    _hip.SIGNATURES.pop(_name)
from bench import build_model
from ppde_amd.sampler import Chains
m, wt, J, h, i0, Lp, cnn = build_model("potts", "cuda:0", "PABP")
n, warm = 128, 200
out = {}
for reuse in (False, True):
    ch = Chains(m, n, warm + 5 * 2000 + 50 * 20 + 8, 2, 0, False, i0, i0 + Lp - 1, 1, 1, reuse_grad=reuse, random_chain=0, use_graph=True, seed=1)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch.run(warm); ch.sync()
    for blocks, steps, tag in ((5, 2000, "long"), (50, 20, "short")):
        dts = []
        for _ in range(blocks):
            torch.cuda.synchronize(); t0 = time.perf_counter(); ch.run(steps); ch.sync(); torch.cuda.synchronize()
            dts.append(time.perf_counter() - t0)
        out[f"us_{tag}_{'reuse' if reuse else 'reeval'}"] = float(np.median(dts)) / steps * 1e6
    res = ch.collect()
    out[f"checksum_{'reuse' if reuse else 'reeval'}"] = float(np.asarray(res["energy_history"], dtype=np.float64).sum())
print("AB " + json.dumps(out))
"""


def main():
    args = sys.argv[1:]
    limit = 240
    if "--limit" in args:
        i = args.index("--limit")
        limit = int(args[i + 1])
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    libs = [os.path.abspath(a) for a in args]
    runs = {0: [], 1: []}
    for rep in range(2):
        for side in (0, 1):
            env = dict(os.environ, PPDE_HIP_LIB=libs[side])
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", CHILD, REPO], capture_output=True, text=True, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("AB ")]
            if r.returncode != 0 or not line:
                print(f"{'AB'[side]} {os.path.basename(libs[side])} run {rep}: status {r.returncode}; stopping here\n{r.stderr[-1500:]}", flush=True)
                sys.exit(1)
            d = json.loads(line[-1][3:])
            runs[side].append(d)
            print(f"{'AB'[side]} {os.path.basename(libs[side])} run {rep}: {json.dumps(d)}", flush=True)
    for key in ("us_long_reeval", "us_short_reeval", "us_long_reuse", "us_short_reuse"):
        a, b = [d[key] for d in runs[0]], [d[key] for d in runs[1]]
        spread = max(abs(a[0] - a[1]), abs(b[0] - b[1]))
        gains = [a[i] - b[i] for i in range(2)]
        gain = sum(gains) / 2
        ok = all(g > 0 for g in gains) and gain >= 3 * spread
        print(f"{key}: A {a[0]:.3f} {a[1]:.3f}  B {b[0]:.3f} {b[1]:.3f}  spread {spread:.3f}  gain of B {gain:.3f} us "
              f"({100 * gain / (sum(a) / 2):.2f} %)  {'>= 3 x spread in both pairings' if ok else 'inside the noise'}")
    same = all(runs[0][0][k] == d[k] for k in ("checksum_reeval", "checksum_reuse") for s in (0, 1) for d in runs[s])
    print("energy-history checksums:", "equal on both sides" if same else "DIFFER")


if __name__ == "__main__":
    main()

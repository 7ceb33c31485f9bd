#!/usr/bin/env python3
"""Records what the chain kernels of a library build compute on the runs of tests/helpers_chain_path.py: path lengths, every
move, accept bits, log_acc, histories, best and final states. tests/test_chain_path_gpu.py compares the built library with the
recording bit for bit, so the file is written from the build a change starts from (PPDE_HIP_LIB selects it):

    PPDE_HIP_LIB=/path/to/parent/libppde_hip.so python scripts/record_chain_bits.py          -> tests/golden/chain_bits_parent.npz
    python scripts/record_chain_bits.py --out some.npz --case b_untraced_reeval [--case ...]   (the test's child process)
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    import helpers_chain_path as hc
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", hc.FIXTURE))
    ap.add_argument("--case", action="append", help="record only these cases (default: all)")
    ap.add_argument("--eager", action="store_true", help="launch every iteration eagerly instead of replaying hipGraphs")
    a = ap.parse_args()
    out = hc.record(a.case, use_graph=not a.eager)
    np.savez_compressed(a.out, **out)
    print(f"recorded {len(out)} arrays of {len(a.case or hc.cases())} runs from "
          f"{os.path.basename(os.environ.get('PPDE_HIP_LIB', 'the shipped library'))}: {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()

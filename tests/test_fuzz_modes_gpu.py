"""Short runs of the mode fuzzer (tests/fuzz_modes.py) on the fixed seed lists of tests/helpers_fuzz_modes.GPU_CASES, each in a fresh
child process (PPDE_GRAPH_LEN and PPDE_CHAIN_SPEC are read once per process), one after the other:
  default_env      the default environment: runs of 6..14 iterations fit no graph segment and are issued eagerly;
  graph_len_4      PPDE_GRAPH_LEN=4: the short runs replay graphs under every dynamics (with recombination where 4 is a multiple of
                   `every`); the script demands that every dynamics replayed some steps;
  general_kernels  PPDE_CHAIN_SPEC=0 on the default and library trials: the general chain kernels in place of the pinned ones;
  patterns         FZ_FORBID=1: the five reversible dynamics x library x allow_native with forbidden patterns built on each
                   configuration's unconstrained reference; veto counters, active words and outcome 4 compared exactly;
  patterns_graph_len_4  the same axes under PPDE_GRAPH_LEN=4: the veto launch inside replayed segments.
tests/test_fuzz_modes_cpu.py shows what these lists cover and that the comparison sees every planted fault."""
import os
import subprocess
import sys

import pytest

import helpers_fuzz_modes as fz

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(fz.GPU_CASES))
def test_fuzz_modes(case):
    c = fz.GPU_CASES[case]
    env = dict(os.environ, FZ_TRIALS=str(c["trials"]), **c["env"])
    if c["dynamics"]:
        env["FZ_DYNAMICS"] = ",".join(c["dynamics"])
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "fuzz_modes.py"), str(c["seed"])], env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-6000:])
    assert "Memory access fault" not in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "failures: 0" in r.stdout

"""The chain kernels' serial path (ppde_amd/csrc/pas.h: propose_body_dev, reverse_rows_dev, accept_body) must keep its bits:
tests/golden/chain_bits_parent.npz holds what the kernels computed BEFORE the path was shortened (recorded by
scripts/record_chain_bits.py from that commit's build), on runs chosen to reach every form of the shared bodies -- one to
three residue groups per thread, paths of up to nine and of more than 64 moves, the mutation cap's flip, the pinned and the general instantiations,
a design library, reversible mode, tempering. Every recorded array is compared through integer views of its floats."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_chain_path as hc
import ppde_oracle as orc
from helpers import GOLDEN, device_noise, oracle_energy

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = hc.cases()


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, hc.FIXTURE), allow_pickle=False)


def _equal_bits(got, fx, name):
    keys = sorted(k for k in fx.files if k.startswith(name + "/"))
    assert keys and {k.split("/", 1)[1] for k in keys} == set(got), (name, keys, sorted(got))
    for k in keys:
        a, b = hc.bits(got[k.split("/", 1)[1]]), hc.bits(fx[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), f"{k}: {int((a != b).sum())} of {a.size} values differ from the parent commit's"


def test_the_fixture_holds_every_case(parent):
    assert {k.split("/", 1)[0] for k in parent.files} == set(CASES)
    for name, spec in CASES.items():
        if spec.get("trace", True):
            U = parent[f"{name}/U"]
            if "longest" in spec:
                assert U.max() >= spec["longest"], name
                continue
            assert U.min() >= 1 and U.max() == 2 * spec["pas"] - 1, name       # the longest path of the case was drawn
            assert 0 < parent[f"{name}/accepted"].mean() < 1, name
    # the cap was reached (the flip of its mask inside a path) where a case sets one
    flat = parent["a_pas5_nmut3_reeval/flat"]
    assert (flat >= 0).sum(1).max() == 9


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_bits_equal_the_parent_commits(parent, name):
    _equal_bits(hc.run_case(CASES[name]), parent, name)


def test_pinned_and_general_kernels_keep_the_same_bits(parent, tmp_path):
    """Case b without trace buffers runs the pinned k_propose<1,false,13> / k_accept<1,13,true> / k_accept_propose<1,5>; the same
    run in a fresh child process with PPDE_CHAIN_SPEC=0 (read once per process) runs the general kernels. Both sides equal the
    parent's recording (above, for this process's side) and each other, and the traced run's histories too."""
    names = ["b_untraced_reeval", "b_untraced_reuse"]
    out = str(tmp_path / "general.npz")
    cmd = [sys.executable, os.path.join(REPO, "scripts", "record_chain_bits.py"), "--out", out] + [x for n in names for x in ("--case", n)]
    r = subprocess.run(cmd, env=dict(os.environ, PPDE_CHAIN_SPEC="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    general = np.load(out, allow_pickle=False)
    for name in names:
        pinned = hc.run_case(CASES[name])
        _equal_bits({k.split("/", 1)[1]: general[k] for k in general.files if k.startswith(name + "/")}, parent, name)
        traced = name.replace("untraced", "traced")
        for k, v in pinned.items():
            assert np.array_equal(hc.bits(v), hc.bits(general[f"{name}/{k}"])), (name, k)
            assert np.array_equal(hc.bits(v), hc.bits(parent[f"{traced}/{k}"])), (name, k)


@pytest.mark.parametrize("reuse", [False, True])
def test_paths_through_two_dominant_residues_in_different_waves(reuse):
    """A field of +30 on one letter of residues 3 and 40 (waves 0 and 3 of the accept kernel's block): paths of two and three moves
    visit both, in either order, so a wave's reverse rows change at the second or third row only -- the rows before it are copies
    of their predecessor (reverse_rows_dev). nmut_threshold 2 sends a chain that holds both back to the wild type, so the two
    moves are there to be taken again in every iteration. Oracle fed the device's own noise: draws and accept bits exact. log_acc
    is a sum of an energy difference and 2 U logarithms of fp32 quotients: |err| <= e_tol of the two energies (5e-6 max(1, |e|) each, this
    suite's energy tolerance) + 2e-4 (the bound tests/test_hip_parity.py puts on log_acc for paths of up to five moves)."""
    m, wt, J, h, plus = hc.two_dominant_sites_model()
    L, Lp, n, T, pas, nmut = wt.shape[0], J.shape[0], 4, 24, 2, 2
    from ppde_amd.sampler import Chains
    ch = Chains(m, n, T, pas, nmut, False, 0, Lp - 1, 1, 1, reuse_grad=reuse, trace=True, random_chain=0, seed=515, use_graph=False)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    en = oracle_energy(J, h, 0, wt, None, 0.0)
    ref = orc.run(en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, 0, Lp - 1, pas, nmut, False, trace=True)
    eh = ref["energy_history"].numpy()
    orders = set()
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (reuse, t, s)
        for b in range(n):
            seen = [int(f) // 20 for f in tr["flat"][t, :U[b], b] if int(f) // 20 in (plus[0][0], plus[1][0])]
            orders.update(zip(seen, seen[1:]))
        la, lr = tr["log_acc"][t], ref["traces"][t]["log_acc"].numpy()
        tol = 2e-4 + 2 * 5e-6 * np.maximum(1.0, np.abs(eh[t:t + 2]).max(0))
        print(f"[two dominant residues] reuse {int(reuse)} iteration {t}: max |log_acc err| {np.abs(la - lr).max():.3e}, tolerance {tol.min():.3e}")
        assert (np.abs(la - lr) <= tol).all(), (reuse, t, la, lr)
    assert {(plus[0][0], plus[1][0]), (plus[1][0], plus[0][0])} <= orders      # both residues on one path, in both orders
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert (np.abs(res["energy_history"] - eh) <= 5e-6 * np.maximum(1.0, np.abs(eh))).all()
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())

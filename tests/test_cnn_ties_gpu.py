"""Directed EXACT arg-max ties through the supervised CNN's kernels: the input gradient must sit on the first-row vertex.

The max over sequence positions routes each feature's decoder weight to one row; on a tie the kernels mean to take the first row
at every merge level (cnn.h: within a lane over its rows, across the four lane groups of a wave, within a 64-row forward chunk,
and across the chunks in k_cnn_bwd_chunk). The states are helpers.tied_states: the wild type with 0-8 random mutations and one
5- or 6-mer copied to a second place, which ties the rows of the two copies exactly for every feature whose maximum sits there
(h2[t, f] depends only on the K-mer at row t). Which chain covers what -- chain b carries placement b % len(TIE_PLACEMENTS[tag]),
(first row, second row, length, source copy), rows of T = L - 4:

  PABP (single launch, six row tiles; seeded and trained networks), chains b % 8 =
    0 (34, 40)  both copies in the same 16-row tile, lane groups 0 and 2
    1 (18, 34)  the same lane and the same j in tiles 1 and 2: decided by the lane's own strict > over its rows
    2 (15, 32)  tiles 0 and 2 with the FIRST row in the higher lane group (3 against 0): decided by the shuffle merge's row test
    3 (52, 73)  a 6-mer: two consecutive tied rows, different tiles and lane groups
    4 (53, 91)  the second copy on the last row T - 1 (the partly filled last tile)
    5 (62, 90)  a 6-mer up to the last row
    6 (0, 64)   row 0 and tile 4
    7 (16, 35)  lane group 0 twice, different j and tile
  UBE4B (trained; the general seven-tile instantiation of the fused launch for small batches, two forward chunks for the 130),
  chains b % 8 =
    0 (21, 27) same tile   1 (22, 54) same lane, tiles 1 / 3   2 (31, 50) first row in the higher lane group
    3 (63, 70) the first copy on the LAST row of forward chunk 0, the second in chunk 1
    4 (26, 84) 6-mer, chunks 0 / 1   5 (54, 99) second copy on the last row (seventh tile)   6 (0, 70) row 0 / chunk 1
    7 (61, 98) 6-mer up to the last row
  GFP (trained; the chunk kernels, four forward chunks of 64 rows), chains b % 10 =
    0 (63, 70) last row of chunk 0 / chunk 1     1 (60, 200) chunks 0 / 3     2 (127, 133) 6-mer whose first copy straddles chunks 1 | 2
    3 (100, 232) second copy on the last row, chunk 3     4 (32, 40) same tile     5 (3, 19) same lane, tiles 0 / 1 of one chunk
    6 (14, 33) first row in the higher lane group     7 (70, 130) chunks 1 / 2     8 (5, 192) 6-mer, chunk 0 / first rows of chunk 3
    9 (0, 227) row 0 / 6-mer up to the last row

tests/test_tie_reference_cpu.py proves without a GPU that every placement ties features in some chain, that no chain is
unresolved, that the option matrix has full rank and that the fp32 oracle sits within 4.9e-7 of its vertex (relative to the
chain's largest entry). The tolerance here is test_cnn_weight_magnitudes': 4e-6 of the chain's OWN largest gradient entry."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppde_oracle as orc
from helpers import (REAL_PROTEINS, cnn_grad_decompose, cnn_grad_match, cnn_grad_vertex, device_noise, oracle_energy, tie_networks,
                     tied_states)
from test_hip_parity import e_tol, hip_model, observed
from ppde_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("pabp", False), ("pabp", True), ("ube4b", True), ("gfp", True)]
N, LAM, RTOL = 130, 5.0, 4e-6


def case_key(tag, trained):
    return f"{tag}_{'trained' if trained else 'seeded'}"


def tie_model(tag, trained):
    """(model pieces, states) of one directed case: Potts couplings as in test_repeated_evaluations_are_bit_identical"""
    _, seq, (i0, Lp) = synthetic.PROTEINS[REAL_PROTEINS[tag]]
    J, h = synthetic.make_potts(Lp, seed=1234)
    idx, which, wt = tied_states(tag, N)
    return J, h, i0, Lp, wt, tie_networks(tag, trained), idx


_TIE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np, torch
from test_cnn_ties_gpu import CASES, LAM, case_key, tie_model
from test_hip_parity import hip_model
out = {}
for tag, trained in CASES:
    J, h, i0, Lp, wt, cnn, idx = tie_model(tag, trained)
    m = hip_model(J, h, i0, wt, cnn, LAM)
    for which in (2, 3):
        for nb in (1, 3, 130):
            e, f, g = m.energy_grad(torch.as_tensor(idx[:nb]).cuda(), which)
            for k, v in zip("efg", (e, f, g)): out[f"{case_key(tag, trained)}.{k}{which}_{nb}"] = v.cpu().numpy()
    m.close()
np.savez(sys.argv[2], **out)
"""

_child_failed = []


def run_child(argv, env, timeout):
    """One child process with its own time limit; after a child has failed, timed out or died nothing further is started."""
    assert not _child_failed, f"an earlier child process failed ({_child_failed[0]}): nothing further is run on the GPU"
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        _child_failed.append(f"timeout {env}")
        raise
    if r.returncode != 0:
        _child_failed.append(f"exit status {r.returncode} {env}")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


FORMS = (("default", {}), ("general", {"PPDE_CNN_SPEC": "0"}), ("unfused", {"PPDE_FUSE_EXPERTS": "0"}), ("chunks256", {"PPDE_CNN_CHUNK_512": "0"}),
         ("fp32", {"PPDE_CNN_BF16": "0"}))


@pytest.fixture(scope="module")
def forms():
    res = {}
    with tempfile.TemporaryDirectory() as d:
        script = os.path.join(d, "tie_child.py")
        open(script, "w").write(_TIE_CHILD)
        for name, env in FORMS:
            out = os.path.join(d, name + ".npz")
            run_child([sys.executable, script, REPO, out], env, 400)
            res[name] = dict(np.load(out))
    return res


_refs = {}


def reference(tag, trained):
    """Per chain: the fp64 decomposition, the fp32 oracle's fitness / energy and its gradient of the Potts expert alone."""
    key = case_key(tag, trained)
    if key not in _refs:
        J, h, i0, Lp, wt, cnn, idx = tie_model(tag, trained)
        en = oracle_energy(J, h, i0, wt, cnn, LAM)
        ix = torch.as_tensor(idx.astype(np.int64))
        eo, fo, go = en.energy_grad(ix)
        _, gc = en.cnn.fit_grad(ix)
        potts = go.double().numpy() - LAM * gc.double().numpy()
        _refs[key] = dict(idx=idx, cnn=cnn, decs=[cnn_grad_decompose(cnn, idx[b]) for b in range(N)], eo=eo.numpy(), fo=fo.numpy(), potts=potts)
    return _refs[key]


def check_first_row_vertices(res, label):
    """(a) and (b) on one library / form: every chain's gradient on the vertex that takes the FIRST row in every exact tie (near
    ties and ReLU kinks, where two correct implementations may differ, as the search finds them), within 4e-6 of the chain's own
    largest entry; the fitness within 5e-6 (relative beyond 1, as test_energy_grad_shapes has it)."""
    for tag, trained in CASES:
        key, ref = case_key(tag, trained), reference(tag, trained)
        fo = ref["fo"]
        for which, lam in ((2, 1.0), (3, LAM)):
            g = res[f"{key}.g{which}_{N}"].astype(np.float64)
            errs, tols, moved, exact_groups = np.zeros(N), np.zeros(N), 0, 0
            for b in range(N):
                dec = ref["decs"][b]
                assert not dec["unresolved"], (key, b)
                other = ref["potts"][b] if which == 3 else 0.0
                _, picks, _, _ = cnn_grad_match((g[b] - other) / lam, ref["cnn"], ref["idx"][b], dec=dec)
                picks = [0 if ex else k for k, ex in zip(picks, dec["exact"])]      # an exact tie goes to the first row: no search there
                v = other + lam * cnn_grad_vertex(dec, picks)
                errs[b], tols[b] = np.abs(g[b] - v).max(), RTOL * np.abs(v).max()
                moved += any(picks)
                exact_groups += sum(dec["exact"])
            print(f"[ties] {label}{key} which {which}: {exact_groups} exact ties in {N} chains, {moved} chain(s) took another row in a NEAR tie")
            assert observed(f"{label}{key}:which{which}:grad", errs, tols) <= 1.0, (key, which, np.argmax(errs / tols))
            f = res[f"{key}.f{which}_{N}"]
            assert observed(f"{label}{key}:which{which}:fit", np.abs(f - fo), 5e-6 * np.maximum(1.0, np.abs(fo))) <= 1.0
        e3 = res[f"{key}.e3_{N}"]
        assert observed(f"{label}{key}:e", np.abs(e3 - ref["eo"]), e_tol(ref["eo"], LAM) + 4e-6 * LAM * np.maximum(1.0, np.abs(fo))) <= 1.0
        assert np.array_equal(res[f"{key}.e2_{N}"], res[f"{key}.f2_{N}"])


def test_exact_ties_take_the_first_row(forms):
    """(a), (b): the default kernels (two fp16 terms per product)"""
    check_first_row_vertices(forms["default"], "ties_")


def test_exact_ties_take_the_first_row_with_fp32_contractions(forms):
    """(d): PPDE_CNN_BF16=0, the exact-fp32 matrix-core contractions, land on the first-row vertex as well"""
    check_first_row_vertices(forms["fp32"], "ties_fp32_")


def test_launch_forms_give_the_same_bits_on_tied_states(forms):
    """(c): the general instantiations, the unfused launch and the 256-thread chunk kernels compute the default form's bits"""
    for name in ("general", "unfused", "chunks256"):
        assert forms[name].keys() == forms["default"].keys()
        for k, v in forms["default"].items():
            assert np.isfinite(v).all() and np.array_equal(v, forms[name][k]), (name, k)


def test_a_tied_chain_does_not_depend_on_its_batch(forms):
    """(f): batches of 1, 3 and 130 chains (other chain-group counts and launch shapes, chunked instead of single launch)"""
    for name, res in forms.items():
        for tag, trained in CASES:
            key = case_key(tag, trained)
            for which in (2, 3):
                for k in "efg":
                    big = res[f"{key}.{k}{which}_{N}"]
                    for nb in (1, 3):
                        assert np.array_equal(res[f"{key}.{k}{which}_{nb}"], big[:nb]), (name, key, which, k, nb)


@pytest.mark.parametrize("tag,trained", CASES)
def test_repeated_evaluations_of_tied_states_are_bit_identical(tag, trained):
    """(e): 200 evaluations of the tied batch give the same bits every time (a tie decided by timing would not)"""
    assert not _child_failed, "a child process failed: nothing further is run on the GPU"
    J, h, i0, Lp, wt, cnn, idx = tie_model(tag, trained)
    m = hip_model(J, h, i0, wt, cnn, LAM)
    x = torch.as_tensor(idx).cuda()
    e0, f0, g0 = [t.cpu().numpy().copy() for t in m.energy_grad(x, 3)]
    assert np.isfinite(e0).all() and np.isfinite(g0).all()
    for rep in range(200):
        e, f, g = [t.cpu().numpy() for t in m.energy_grad(x, 3)]
        assert np.array_equal(e, e0) and np.array_equal(f, f0) and np.array_equal(g, g0), rep
    m.close()


def test_sampler_run_from_tied_states():
    """16 chains, 25 device-RNG steps started FROM tied states on the trained PABP networks, against the oracle fed the device's
    noise: draws, accept bits and best states exact (no mutation cap, so that the chains stay near the tied states)."""
    from ppde_amd.sampler import Chains
    assert not _child_failed, "a child process failed: nothing further is run on the GPU"
    J, h, i0, Lp, wt, cnn, idx = tie_model("pabp", True)
    m = hip_model(J, h, i0, wt, cnn, LAM)
    n, T, pas = 16, 25, 2
    start = idx[:n]
    ch = Chains(m, n, T, pas, 0, False, i0, i0 + Lp - 1, 3, 1, trace=True, random_chain=0, seed=77, use_graph=False)
    ch.init(torch.as_tensor(start).cuda())
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    ref = orc.run(oracle_energy(J, h, i0, wt, cnn, LAM), start.astype(np.int64), wt, lambda t: noise[t], T, i0, i0 + Lp - 1, pas, 0, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    eh, fh = ref["energy_history"].numpy(), ref["fitness_history"].numpy()
    assert observed("ties_run:energy_history", np.abs(res["energy_history"] - eh), e_tol(eh, LAM) + 4e-6 * LAM * np.maximum(1.0, np.abs(fh))) <= 1.0


_REPLAY_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
from ppde_amd import _hip
assert _hip.LIB_PATH.endswith("libppde_hip_exact.so"), _hip.LIB_PATH
import test_hip_parity as t
for name in t.RUNS_Q:
    for reuse in (True, False):
        t.test_sampler_replays_reference_trajectory(name, reuse)
        print("replayed", name, reuse, flush=True)
assert len(t.RUNS_Q) >= 1
"""


def test_exact_split_library():
    """ppde_amd/libppde_hip_exact.so (-DCNN_SPLIT=3: every product of the CNN's contractions exact, three bf16 terms per operand;
    built by __graft_entry__.build()) in fresh child processes with PPDE_HIP_LIB set: the trained networks of the three proteins
    against the reference's outputs, the directed ties (a) and (b), and the recorded TOY24 trajectories."""
    from helpers import load
    from test_hip_parity import _TRAINED_KNOBS, _check_trained
    lib = os.path.join(REPO, "ppde_amd", "libppde_hip_exact.so")
    assert os.path.exists(lib), f"{lib} is missing: __graft_entry__.build() builds it (python -c 'from ppde_amd import build; build.build_exact()')"
    env = {"PPDE_HIP_LIB": lib}
    with tempfile.TemporaryDirectory() as d:
        for name, text in (("trained", _TRAINED_KNOBS), ("ties", _TIE_CHILD), ("replay", _REPLAY_CHILD)):
            open(os.path.join(d, name + ".py"), "w").write(text)
        run_child([sys.executable, os.path.join(d, "trained.py"), REPO, os.path.join(d, "trained.npz")], env, 400)
        trained = dict(np.load(os.path.join(d, "trained.npz")))
        run_child([sys.executable, os.path.join(d, "ties.py"), REPO, os.path.join(d, "ties.npz")], env, 400)
        ties = dict(np.load(os.path.join(d, "ties.npz")))
        r = run_child([sys.executable, os.path.join(d, "replay.py"), REPO], env, 600)
        assert r.stdout.count("replayed") >= 2, r.stdout[-2000:]
    for tag in ("pabp", "ube4b", "gfp"):
        _check_trained(tag, load(f"real_{tag}.npz"), {k.split(".", 1)[1]: v for k, v in trained.items() if k.startswith(tag + ".")}, "", prefix="exact_split:")
    check_first_row_vertices(ties, "exact_split:ties_")

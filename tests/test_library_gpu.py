"""Design libraries on the GPU (ppde_chains_set_library): the proposal kernels against the masked reference of
tests/helpers_library.py -- replayed noise (flat race), the device RNG (two-level draw) in every form of the chain kernels,
the exact law on an enumerable state space, and the interfaces above them (C ABI errors, sharding, streams, the driver).

Tolerances are tests/test_hip_parity.py's for the same quantities: draws, accept bits and best states exact; energy histories
2e-5, fitness 5e-6, log acceptance ratios 2e-4."""
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppde_oracle as orc
import helpers_library as hl
from helpers import device_noise, load, model_from_fixture
from ppde_amd import library as dl
from ppde_amd import synthetic
from ppde_amd.encoding import ALPHABET

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")


def _chains(m, case, n, T, pas, nmut, paper, rng_mode, lib, lo=None, hi=None, x0=None, set_lib=True, **kw):
    from ppde_amd.sampler import Chains
    lo = case["i0"] if lo is None else lo
    hi = case["i0"] + case["Lp"] - 1 if hi is None else hi
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", 99)
    ch = Chains(m, n, T, pas, nmut, paper, lo, hi, 3 if case.get("cnn") is not None else 1, rng_mode, **kw)
    if set_lib:
        ch.set_library(lib)
    x0 = np.tile(case["wt"], (n, 1)) if x0 is None else x0
    ch.init(torch.as_tensor(x0).cuda())
    return ch


def _feed(ch, noise):
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _assert_same(a, b, tr_a=None, tr_b=None, label=""):
    for k in RESULT_KEYS:
        assert np.array_equal(a[k], b[k]), (label, k)
    if tr_a is not None:
        for k in ("flat", "accepted", "log_acc", "U"):
            assert np.array_equal(tr_a[k], tr_b[k]), (label, k)


def _assert_against_reference(tr, res, ref, noise, T, lib, check_U=False):
    ok = dl.as_bool(lib).reshape(-1)
    for t in range(T):
        U = noise[t][0].numpy()
        if check_U:
            assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
            assert ok[tr["flat"][t, s][act]].all()
        assert np.allclose(tr["log_acc"][t], ref["traces"][t]["log_acc"].numpy(), atol=2e-4), t
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.abs(res["fitness_history"] - ref["fitness_history"].numpy()).max() <= 5e-6


# ------------------------------------------------------------------------------------------------ 1. all letters = no library
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_all_letters_library_gives_the_bits_of_no_library(rng_mode, reuse):
    c = hl.toy24()
    m = hl.hip_model_of(c)
    n, T, pas, nmut = 16, 12, 2, 3
    torch.manual_seed(23)
    noise = [orc.draw_noise_torch(n, c["L"] * 20, pas) for _ in range(T)]
    out = []
    for with_lib in (False, True):
        ch = _chains(m, c, n, T, pas, nmut, False, rng_mode, dl.full_library(c["L"]), set_lib=with_lib, trace=True, reuse_grad=reuse,
                     use_graph=False)
        if rng_mode == 0:
            _feed(ch, noise)
        else:
            ch.run(T)
        out.append((ch.collect(), ch.trace()))
        ch.close()
    _assert_same(out[0][0], out[1][0], out[0][1], out[1][1])
    assert (out[0][1]["accepted"] != 0).any()
    m.close()


# ------------------------------------------------------------------------------------------------ 2. replay, flat race
@pytest.fixture(scope="module")
def toy():
    c = hl.toy24()
    lib = hl.seeded_library(c["wt"], c["i0"], c["i0"] + c["Lp"] - 1, seed=41)
    return c, lib, hl.oracle_energy_of(c)


@pytest.mark.parametrize("paper", [False, True])
@pytest.mark.parametrize("nmut", [0, 3])
@pytest.mark.parametrize("pas", [1, 3])
def test_replay_against_the_masked_reference(toy, pas, nmut, paper):
    c, lib, en = toy
    n, T, lo, hi = 16, 20, c["i0"], c["i0"] + c["Lp"] - 1
    torch.manual_seed(1000 + 10 * pas + nmut + int(paper))
    noise = [orc.draw_noise_torch(n, c["L"] * 20, pas) for _ in range(T)]
    ref = hl.masked_run(lib, en, np.tile(c["wt"].astype(np.int64), (n, 1)), c["wt"], lambda t: noise[t], T, lo, hi, pas, nmut, paper, trace=True)
    m = hl.hip_model_of(c)
    res = []
    for reuse in (True, False):
        ch = _chains(m, c, n, T, pas, nmut, paper, 0, lib, trace=True, reuse_grad=reuse)
        _feed(ch, noise)
        tr, r = ch.trace(), ch.collect()
        _assert_against_reference(tr, r, ref, noise, T, lib)
        res.append((r, tr))
        ch.close()
    _assert_same(res[0][0], res[1][0], res[0][1], res[1][1])
    frozen = np.flatnonzero(lib == 0)
    assert (res[0][0]["best_idx"][:, frozen] == c["wt"][frozen][None]).all()
    m.close()


# ------------------------------------------------------------------------------------------------ 3. device RNG, two-level draw
def _device_rng_case(c, lib, n, T, pas, nmut, lo, hi):
    en = hl.oracle_energy_of(c)
    m = hl.hip_model_of(c)
    ch = _chains(m, c, n, T, pas, nmut, False, 1, lib, lo, hi, trace=True, reuse_grad=False, use_graph=False)
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    ref = hl.masked_run(lib, en, np.tile(c["wt"].astype(np.int64), (n, 1)), c["wt"], lambda t: noise[t], T, lo, hi, pas, nmut, False, trace=True)
    _assert_against_reference(tr, res, ref, noise, T, lib, check_U=True)
    for reuse in (False, True):                                  # untraced, graph-replayed, both evaluation policies
        ch3 = _chains(m, c, n, T, pas, nmut, False, 1, lib, lo, hi, trace=False, reuse_grad=reuse, use_graph=True)
        ch3.run(T)
        res3 = ch3.collect()
        assert ch3.graph_stats()["replayed_steps"] == T
        _assert_same(res, res3, label=f"reuse={reuse}")
        ch3.close()
    ch.close()
    m.close()
    return tr


@pytest.mark.parametrize("nmut", [0, 3])
def test_device_rng_against_the_masked_reference(toy, nmut):
    c, lib, _ = toy
    _device_rng_case(c, lib, 64, 20, 2, nmut, c["i0"], c["i0"] + c["Lp"] - 1)


@pytest.mark.parametrize("L,i0,Lp,first_open", [(70, 60, 8, 64), (104, 40, 16, 40), (237, 200, 16, 200)])
def test_device_rng_in_every_form_of_the_chain_kernels(L, i0, Lp, first_open):
    """Potts only: L = 70 with every open residue at 64 or beyond (the second round of the residue race), L = 104 and L = 237
    with a 16-residue window (two and three logit groups per thread). No graph segment fits T = 6, so the untraced runs here
    are issued eagerly; the next test replays the two long geometries from graphs."""
    c = hl.potts_case(L, i0, Lp, seed=L)
    hi = i0 + Lp - 1
    lib = hl.seeded_library(c["wt"], first_open, hi, seed=L + 1)
    assert dl.open_sites(lib).min() >= first_open
    n, T, pas = 8, 6, 2
    en = hl.oracle_energy_of(c)
    m = hl.hip_model_of(c)
    ch = _chains(m, c, n, T, pas, 0, False, 1, lib, i0, hi, trace=True, reuse_grad=False, use_graph=False)
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, pas)
    ref = hl.masked_run(lib, en, np.tile(c["wt"].astype(np.int64), (n, 1)), c["wt"], lambda t: noise[t], T, i0, hi, pas, 0, False, trace=True)
    _assert_against_reference(tr, res, ref, noise, T, lib, check_U=True)
    for reuse in (False, True):
        ch3 = _chains(m, c, n, T, pas, 0, False, 1, lib, i0, hi, trace=False, reuse_grad=reuse, use_graph=True)
        ch3.run(T)
        _assert_same(res, ch3.collect(), label=f"reuse={reuse}")
        ch3.close()
    m.close()


@pytest.mark.parametrize("L,i0,Lp", [(104, 40, 16), (237, 200, 16)])
def test_graph_replay_of_the_library_kernels_with_two_and_three_groups_per_thread(L, i0, Lp):
    """The same two geometries at T = 20, the shortest run a graph segment fits: untraced runs replayed from hipGraphs
    (`replayed_steps == T`) under both evaluation policies, bit-equal to the traced eager run that the case above ties to the
    masked reference."""
    c = hl.potts_case(L, i0, Lp, seed=L)
    hi = i0 + Lp - 1
    lib = hl.seeded_library(c["wt"], i0, hi, seed=L + 1)
    n, T, pas = 8, 20, 2
    m = hl.hip_model_of(c)
    ch = _chains(m, c, n, T, pas, 0, False, 1, lib, i0, hi, trace=True, reuse_grad=False, use_graph=False)
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    assert ch.graph_stats()["replayed_steps"] == 0 and tr["accepted"].sum() > 0
    drawn = tr["flat"][tr["flat"] >= 0]
    assert dl.as_bool(lib).reshape(-1)[drawn].all()
    for reuse in (False, True):
        ch3 = _chains(m, c, n, T, pas, 0, False, 1, lib, i0, hi, trace=False, reuse_grad=reuse, use_graph=True)
        ch3.run(T)
        assert ch3.graph_stats()["replayed_steps"] == T
        _assert_same(res, ch3.collect(), label=f"reuse={reuse}")
        ch3.close()
    ch.close()
    m.close()


def test_entries_masked_only_by_the_range_keep_the_floor_on_the_device(toy):
    """A library that opens residues OUTSIDE [min_pos, max_pos]: their entries are masked by the range alone, so they keep the
    reference's 2^-23 floor and can be drawn, while an entry the library forbids cannot, whatever the noise. Replay mode with
    the first race of every iteration steered: in even chains the variate of an open-but-masked entry is made tiny (it must win,
    with log-probability log(2^-23 / sum)), in odd chains that of a forbidden entry (it must never be drawn). Everything is
    compared with the masked reference on the same noise."""
    c, lib0, en = toy
    lo, hi, wt, L = c["i0"], c["i0"] + c["Lp"] - 1, c["wt"], c["L"]
    lib = lib0.copy()
    lib[1] = dl.ALL_LETTERS                                             # open, below the range
    lib[22] = np.uint32((1 << int(wt[22])) | (1 << ((int(wt[22]) + 3) % 20)))   # open with two letters, above the range
    floor_entry = 1 * 20 + (int(wt[1]) + 5) % 20
    forbidden_entry = 22 * 20 + (int(wt[22]) + 7) % 20
    ok = dl.as_bool(lib).reshape(-1)
    assert ok[floor_entry] and not ok[forbidden_entry] and not (lo <= 1 <= hi) and not (lo <= 22 <= hi)
    n, T, pas = 16, 8, 2
    torch.manual_seed(77)
    noise = []
    for _ in range(T):
        U, q, u = orc.draw_noise_torch(n, L * 20, pas)
        q[0, 0::2, floor_entry] = 1e-30
        q[0, 1::2, forbidden_entry] = 1e-30
        noise.append((U, q, u))
    ref = hl.masked_run(lib, en, np.tile(wt.astype(np.int64), (n, 1)), wt, lambda t: noise[t], T, lo, hi, pas, 0, False, trace=True)
    m = hl.hip_model_of(c)
    for reuse in (True, False):
        ch = _chains(m, c, n, T, pas, 0, False, 0, lib, trace=True, reuse_grad=reuse)
        _feed(ch, noise)
        tr, res = ch.trace(), ch.collect()
        _assert_against_reference(tr, res, ref, noise, T, lib)
        assert (tr["flat"][:, 0, 0::2] == floor_entry).all()            # the floor entry wins where it is steered ...
        assert not (tr["flat"] == forbidden_entry).any()                # ... the forbidden one nowhere
        ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 4. the law
_LAW = {}


def _law_kernel(nmut):
    if nmut not in _LAW:
        c = hl.law_case()
        c = dict(c, cnn=None, lamda=0.0)
        K, states, index = hl.exact_library_kernel(hl.oracle_energy_of(c), c["wt"], c["allowed"], 1, 0, c["L"] - 1, nmut)
        _LAW[nmut] = (c, K, states, index)
    return _LAW[nmut]


@pytest.mark.parametrize("nmut", [0, 2])
def test_law_under_a_library(nmut):
    """L = 7, Potts window 0..5, residues 2 and 3 open with 7 and 5 letters, single moves: 2^16 chains from the wild type after
    T = 1, 2, 12 iterations against the enumerated kernel's power (Pearson chi-square, merge floor 8, bound df + 5 sqrt(2 df),
    df >= 10 -- tests/test_sampler_law.py's), both evaluation policies at T = 2; and not one chain on a forbidden state."""
    c, K, states, index = _law_kernel(nmut)
    assert np.abs(K.sum(1) - 1.0).max() <= 1e-6
    m = hl.hip_model_of(c)
    n, S, L = 1 << 16, states.shape[0], c["L"]
    start = index[(int(c["wt"][2]), int(c["wt"][3]))]
    x0 = np.tile(states[start].numpy().astype(np.uint8), (n, 1))
    for T in (1, 2, 12):
        Kt = np.linalg.matrix_power(K, T)[start]
        for reuse in ((True, False) if T == 2 else (True,)):
            ch = _chains(m, c, n, T, 1, nmut, False, 1, c["allowed"], 0, L - 1, x0=x0, random_chain=-1, seed=977 + 13 * T + nmut, reuse_grad=reuse)
            ch.run(T)
            ch.sync()
            idx = ch.peek()["idx"]
            ch.close()
            cells, forbidden = hl.state_cells(idx, c["allowed"], index, states[start].numpy())
            assert forbidden == 0
            chi2, df = hl.chi_square(np.bincount(cells, minlength=S).astype(np.float64), n * Kt)
            print(f"library law: nmut={nmut} T={T} reuse={reuse}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
            assert df >= 10, "the case must spread over enough cells to test anything"
            assert chi2 < hl.chi_square_bound(df), (nmut, T, reuse, chi2, df)
    m.close()


# ------------------------------------------------------------------------------------------------ 5. never outside
def test_no_draw_and_no_state_ever_leaves_the_library():
    """PABP geometry, Potts + CNN, 128 chains, 200 iterations on the device RNG from graphs, no cap, the FULL position range:
    the library alone confines the run."""
    fx = load("ops_pabp_lam5.npz")
    J, h, i0, wt, cnn = model_from_fixture(fx)
    c = dict(L=wt.shape[0], Lp=J.shape[0], i0=i0, wt=wt, J=J, h=h, cnn=cnn, lamda=5.0)
    lib = hl.seeded_library(wt, i0, i0 + c["Lp"] - 1, seed=96)
    ok = dl.as_bool(lib)
    m = hl.hip_model_of(c)
    n, T, L = 128, 200, c["L"]
    ch = _chains(m, c, n, T, 2, 0, False, 1, lib, 0, L - 1, trace=True, use_graph=True, random_chain=5, seed=4242)
    ch.run(T)
    tr, res, pk = ch.trace(), ch.collect(), ch.peek()
    assert ch.graph_stats()["replayed_steps"] == T
    flat = tr["flat"]
    drawn = flat[flat >= 0]
    assert drawn.size >= T * n and ok.reshape(-1)[drawn].all()
    assert tr["accepted"].sum() > 0 and (pk["idx"] != wt[None]).any()
    frozen, opened = np.flatnonzero(lib == 0), np.flatnonzero(lib)
    for name, rows in (("peek", pk["idx"]), ("best", res["best_idx"]), ("random_traj", res["random_traj"])):
        assert (rows[:, frozen] == wt[frozen][None]).all(), name
        assert ok[opened[None, :], rows[:, opened].astype(np.int64)].all(), name
    ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 6. sharding and streams
def test_sharding_and_streams_do_not_change_a_library_run(toy):
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    n, T = 16, 25

    def run(n_, off, **kw):
        ch = _chains(m, c, n_, T, 2, 3, False, 1, lib, chain_offset=off, random_chain=0 if off == 0 else -1, **kw)
        ch.run(T)
        r = ch.collect()
        ch.close()
        return r

    one = run(n, 0)
    a, b = run(8, 0), run(8, 8)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    _assert_same(one, run(n, 0, n_streams=2), label="n_streams=2")
    assert (one["energy_history"][1:] != one["energy_history"][:-1]).any()
    m.close()


# ------------------------------------------------------------------------------------------------ 7. the C ABI's errors
def test_set_library_errors_and_clearing(toy):
    from ppde_amd import _hip
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    lo, hi, wt = c["i0"], c["i0"] + c["Lp"] - 1, c["wt"]
    mk = lambda: Chains(m, 8, 10, 2, 0, False, lo, hi, 3, 1, seed=7, random_chain=0)
    ch = mk()
    bad = lib.copy(); bad[lo] |= np.uint32(1 << 20)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*bit >= 20"):  # (the raw call: Chains.set_library checks this one itself)
        _hip.check(ch.lib.ppde_chains_set_library(ch.handle, _hip.ptr(np.ascontiguousarray(bad))))
    with pytest.raises(ValueError, match="bit >= 20"):            # the Python layer refuses it before the call
        ch.set_library(bad)
    s = int(dl.open_sites(lib)[0])
    bad = lib.copy(); bad[s] = np.uint32(1 << ((int(wt[s]) + 1) % 20))
    with pytest.raises(PpdeHipError, match=rf"\[-1\].*residue {s} lacks its wild-type letter"):
        ch.set_library(bad)
    bad = np.zeros(c["L"], np.uint32); bad[lo - 1] = np.uint32(1 << int(wt[lo - 1]))
    with pytest.raises(PpdeHipError, match=r"\[-1\].*no open residue in \[min_pos, max_pos\]"):
        ch.set_library(bad)
    # a refused library leaves the previous state: set, then clear with NULL -> the unrestricted run
    ch.set_library(lib)
    ch.set_library(None)
    x0 = torch.as_tensor(np.tile(wt, (8, 1))).cuda()
    ch.init(x0)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_library(lib)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_library(None)
    ch.run(10)
    free = mk(); free.init(x0); free.run(10)
    _assert_same(ch.collect(), free.collect(), label="cleared")
    lim = mk(); lim.set_library(lib); lim.init(x0); lim.run(10)
    assert not np.array_equal(lim.collect()["energy_history"], free.collect()["energy_history"])
    for x in (ch, free, lim):
        x.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 8. the driver
def test_driver_confines_the_population_to_the_library():
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    wt = np.array([ALPHABET.index(ch) for ch in seq])
    sites_flag, exclude = "5-9,12,15-17", "CM"
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        cmd = [sys.executable, os.path.join(REPO, "scripts", "directed_evolution.py"), "--protein_weights", root, "--protein", "TOY24",
               "--results_path", res, "--device", "cuda:0", "--disable_MSA_transformer_scoring", "--n_chains", "12", "--n_iters", "60",
               "--seed", "3", "--log_every", "25", "--ppde_rng", "philox", "--ppde_sites", sites_flag, "--ppde_exclude", exclude]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = re.search(r"^design library: (\d+) open sites, log10\(size\) = (\d+\.\d+)$", r.stdout, flags=re.M)
        lib = dl.build_library(wt, (i0, i0 + Lp - 1), sites=dl.parse_sites(sites_flag, len(seq)), exclude=exclude)
        assert line and int(line.group(1)) == 9 and abs(float(line.group(2)) - dl.log10_size(lib)) < 1e-3, r.stdout
        out_dir = glob.glob(os.path.join(res, "TOY24", "*"))[0]
        pop = np.load(os.path.join(out_dir, "population.npy")).argmax(-1)
        ok = dl.as_bool(lib)
        frozen, opened = np.flatnonzero(lib == 0), np.flatnonzero(lib)
        assert (pop[:, frozen] == wt[frozen][None]).all()
        assert ok[opened[None, :], pop[:, opened]].all()
        assert (pop != wt[None]).any()
        cfg = json.load(open(os.path.join(out_dir, "config.txt")))
        assert cfg["ppde_sites"] == sites_flag and cfg["ppde_exclude"] == exclude and cfg["ppde_library_file"] is None

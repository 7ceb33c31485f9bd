"""Reversible mode on the GPU (ppde_chains_set_reversible; k_accept_rev, k_accept_propose_rev): the law of the chains against
the enumerated kernel of tests/helpers_reversible.py and against exp(E)/Z itself, replays of the reference on torch's noise
(flat race) and on the device RNG's own (two-level draw), and the interfaces around it.

Tolerances are tests/test_hip_parity.py's for the same quantities: draws, accept bits, best states and trajectories exact
(tests/test_reversible_cpu.py shows that no decision of these runs sits near a tie); log acceptance ratios 2e-4, energy
histories 2e-5, fitness 5e-6. The law tests use tests/test_sampler_law.py's statistic and bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_reversible as hr
from helpers import device_noise
from ppde_amd import library as dl
from ppde_amd import synthetic
from test_hip_parity import observed

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")


def _chains(m, case, n, T, pas, nmut, rng_mode, lib, reversible=True, x0=None, lo=None, hi=None, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", 99)
    lo = 0 if lo is None else lo
    hi = case["L"] - 1 if hi is None else hi
    ch = Chains(m, n, T, pas, nmut, False, lo, hi, 3 if case.get("cnn") is not None else 1, rng_mode, **kw)
    if lib is not None:
        ch.set_library(lib)
    if reversible is not None:
        ch.set_reversible(reversible)
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


def _assert_against_reference(tag, tr, res, ref, noise, T, lib, check_U=False):
    ok = dl.as_bool(dl.full_library(res["best_idx"].shape[1]) if lib is None else lib).reshape(-1)
    for t in range(T):
        U = noise[t][0].numpy()
        if check_U:
            assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
            assert ok[tr["flat"][t, s][act]].all()
    ref_la = np.stack([o["log_acc"].numpy() for o in ref["traces"]])
    la = observed(f"reversible:{tag}:log_acc", np.abs(tr["log_acc"] - ref_la), 2e-4)
    en = observed(f"reversible:{tag}:energy", np.abs(res["energy_history"] - ref["energy_history"].numpy()), 2e-5)
    fi = observed(f"reversible:{tag}:fitness", np.abs(res["fitness_history"] - ref["fitness_history"].numpy()), 5e-6)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy())
    assert la <= 1.0 and en <= 1.0 and fi <= 1.0


# ------------------------------------------------------------------------------------------------ 1. the law
def _one_site_case(L, Lp, i0, site, with_cnn, lam, seed=31):
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, sigma_J=0.3, sigma_h=0.8)
    allowed = np.zeros(L, np.uint32)
    allowed[site] = dl.ALL_LETTERS
    cnn = [synthetic.make_cnn_state(L, s) for s in range(3)] if with_cnn else None
    return dict(L=L, Lp=Lp, i0=i0, wt=wt, J=J, h=h, allowed=allowed, cnn=cnn, lamda=lam, nmut=0)


LAW_CASES = {
    "two residues, 7 and 5 letters, paths of 1-3 moves": lambda: dict(hl.law_case(), cnn=None, lamda=0.0, nmut=0),
    "one residue, all letters, Potts + CNN": lambda: _one_site_case(8, 6, 1, 4, True, 2.0),
    "two residues, 11 letters each, mutation cap 2": hr.cap_case,
    "one residue beyond the first 64 (second round of the residue race)": lambda: _one_site_case(70, 6, 62, 66, False, 0.0),
    # groups per thread = ceil(L * 5 / 512): every case above runs the one-group form
    "L = 104, two groups per thread": lambda: _one_site_case(104, 6, 98, 101, False, 0.0),
    "L = 237, three groups per thread": lambda: _one_site_case(237, 6, 200, 203, False, 0.0),
}
_LAW = {}


def _law(name, pas=2):
    if name not in _LAW:
        c = LAW_CASES[name]()
        K, states, index, e, inside = hr.exact_reversible_kernel(hl.oracle_energy_of(c), c["wt"], c["allowed"], pas, 0, c["L"] - 1, c["nmut"])
        assert np.abs(K[inside].sum(1) - 1.0).max() <= 1e-6
        _LAW[name] = (c, K, states, index, e, inside)
    return _LAW[name]


def _population_against(label, m, c, n, T, pas, start_state, expected, states, index, **kw):
    ch = _chains(m, c, n, T, pas, c["nmut"], 1, c["allowed"], x0=np.tile(start_state.astype(np.uint8), (n, 1)), random_chain=-1, **kw)
    ch.run(T)
    ch.sync()
    idx = ch.peek()["idx"]
    ch.close()
    cells, forbidden = hl.state_cells(idx, c["allowed"], index, start_state)
    assert forbidden == 0
    chi2, df = hl.chi_square(np.bincount(cells, minlength=states.shape[0]).astype(np.float64), n * expected)
    print(f"reversible law, {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)


@pytest.mark.parametrize("name", list(LAW_CASES))
def test_law_of_the_reversible_chains(name):
    """2^16 chains on the device RNG after T = 1 (two start states), 2 (both gradient policies: separate and fused kernels) and
    12 iterations against rows of K^T, K enumerated from the reference at pas_length 2 (paths of 1-3 moves)."""
    c, K, states, index, _, inside = _law(name)
    assert (c["L"] * 5 + 511) // 512 == {104: 2, 237: 3}.get(c["L"], 1)                   # the form of the chain kernels the case runs
    m = hl.hip_model_of(c)
    n = 1 << 16
    rows = np.flatnonzero(inside)
    wt_row = index[tuple(int(c["wt"][p]) for p in np.flatnonzero(c["allowed"]))]
    other = int(rows[(np.searchsorted(rows, wt_row) + len(rows) // 2) % len(rows)])      # a second start state inside the cap
    assert other != wt_row
    for T, start in ((1, wt_row), (1, other), (2, wt_row), (12, other)):
        Kt = np.linalg.matrix_power(K, T)[start]
        for reuse in ((True, False) if T == 2 else (True,)):
            _population_against(f"{name}: T={T} start={start} reuse={reuse}", m, c, n, T, 2, states[start].numpy(), Kt, states, index,
                                seed=977 + 13 * T + start, reuse_grad=reuse)
    m.close()


# ------------------------------------------------------------------------------------------------ 2. equilibrium
def test_the_population_reaches_exp_energy_over_Z():
    """The sentence the mode exists for: after 64 iterations from the wild type the population IS a sample of exp(E)/Z (the
    second eigenvalue of K is below 0.7: K^64 is stationary to 1e-6 in total variation, asserted first on the CPU)."""
    c, K, states, index, e, inside = _law("two residues, 7 and 5 letters, paths of 1-3 moves")
    pi = hr.target_law(e, inside)
    start = index[(int(c["wt"][2]), int(c["wt"][3]))]
    T = 64
    assert np.sort(np.abs(np.linalg.eigvals(K)))[-2] < 0.7
    assert hr.total_variation(np.linalg.matrix_power(K, T)[start], pi) <= 1e-6
    m = hl.hip_model_of(c)
    _population_against("equilibrium against exp(E)/Z, T=64", m, c, 1 << 16, T, 2, states[start].numpy(), pi, states, index, seed=4711)
    m.close()


# ------------------------------------------------------------------------------------------------ 3.-5. replays
@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    return c, lib, hl.oracle_energy_of(c)


def _replay_chains(m, c, lib, k, rng_mode, T=None, **kw):
    return _chains(m, c, k["n"], k["T"] if T is None else T, k["pas"], k["nmut"], rng_mode, lib, lo=c["i0"], hi=c["i0"] + c["Lp"] - 1,
                   seed=k["philox_seed"], **kw)


@pytest.mark.parametrize("name", ["pas2", "pas2_cap3", "pas3", "pas2_nolib"])
def test_replay_of_the_flat_race_against_the_reversible_reference(toy, name):
    """rng_mode 0 on torch's noise, both gradient policies. pas3 reaches paths of five moves: a pass of three reverse rows and
    the remainder pass of two in one path."""
    c, lib, en = toy
    k = hr.REPLAY_CASES[name]
    lib = lib if k.get("library", True) else None
    noise, ref = hr.replay_reference(name, 0, en, c, lib)
    m = hl.hip_model_of(c)
    out = []
    for reuse in (True, False):
        ch = _replay_chains(m, c, lib, k, 0, trace=True, reuse_grad=reuse)
        _feed(ch, noise)
        tr, res = ch.trace(), ch.collect()
        _assert_against_reference(f"{name}:flat:reuse{int(reuse)}", tr, res, ref, noise, k["T"], lib)
        out.append((res, tr))
        ch.close()
    _assert_same(out[0][0], out[1][0], out[0][1], out[1][1])
    wt = torch.as_tensor(c["wt"].astype(np.int64))
    capped = torch.stack([(o["proposal"] != wt).sum(-1) >= (k["nmut"] or 1 << 30) for o in ref["traces"]]).numpy()
    if k["nmut"]:
        assert capped.any() and not out[0][1]["accepted"].astype(bool)[capped].any()        # rejected by the cap ...
    assert out[0][1]["accepted"].any()                                                       # ... and others accepted
    if name == "pas3":
        assert (np.stack([n_[0].numpy() for n_ in noise]) == 5).any()
    m.close()


@pytest.mark.parametrize("name", ["pas2", "pas2_cap3", "pas3", "pas2_nolib"])
def test_replay_of_the_device_rng_against_the_reversible_reference(toy, name):
    """rng_mode 1: the reference fed the device's own noise; then the untraced runs of both gradient policies (fused kernel),
    eager and replayed from hipGraphs, give the traced run's bits."""
    c, lib, en = toy
    k = hr.REPLAY_CASES[name]
    lib = lib if k.get("library", True) else None
    T, lo, hi = k["T_dev"], c["i0"], c["i0"] + c["Lp"] - 1
    m = hl.hip_model_of(c)
    ch = _replay_chains(m, c, lib, k, 1, T=T, trace=True, reuse_grad=False, use_graph=False)
    ch.run(T)
    tr, res = ch.trace(), ch.collect()
    noise = device_noise(ch, T, k["pas"])
    for t, (U, q, u) in enumerate(hr.replay_noise(name, 1, c["L"])):                         # the noise the CPU margins were checked on
        assert np.array_equal(U.numpy(), noise[t][0].numpy()) and np.array_equal(u.numpy(), noise[t][2].numpy())
    ref = hr.reversible_run(en, np.tile(c["wt"].astype(np.int64), (k["n"], 1)), c["wt"], lambda t: noise[t], T, lo, hi, k["pas"], k["nmut"],
                            trace=True, allowed=lib)
    _assert_against_reference(f"{name}:device", tr, res, ref, noise, T, lib, check_U=True)
    assert tr["accepted"].any() and not tr["accepted"].all()
    for reuse in (False, True):
        for graph in (False, True):
            ch3 = _replay_chains(m, c, lib, k, 1, T=T, trace=False, reuse_grad=reuse, use_graph=graph)
            ch3.run(T)
            assert ch3.graph_stats()["replayed_steps"] == (T if graph else 0)
            _assert_same(res, ch3.collect(), label=f"reuse={reuse} graph={graph}")
            ch3.close()
    ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 6. off means off
def test_reversible_off_gives_the_bits_of_a_run_that_never_heard_of_it(toy):
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    n, T = 16, 20
    out = []
    for rev in (None, False, True):
        ch = _chains(m, c, n, T, 2, 3, 1, lib, reversible=rev, lo=c["i0"], hi=c["i0"] + c["Lp"] - 1, trace=True)
        ch.run(T)
        out.append((ch.collect(), ch.trace()))
        ch.close()
    _assert_same(out[0][0], out[1][0], out[0][1], out[1][1], label="set_reversible(False)")
    assert np.array_equal(out[0][1]["flat"][0], out[2][1]["flat"][0])                        # the first forward path is the same one ...
    assert not np.array_equal(out[0][1]["log_acc"], out[2][1]["log_acc"])                    # ... and scored differently
    m.close()


# ------------------------------------------------------------------------------------------------ 7. the C ABI
def test_set_reversible_refusals_and_a_start_state_outside_the_library(toy):
    from ppde_amd._hip import PpdeHipError
    from ppde_amd.sampler import Chains
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    lo, hi, wt = c["i0"], c["i0"] + c["Lp"] - 1, c["wt"]
    n, T = 8, 20
    x0 = np.tile(wt, (n, 1))
    ch = Chains(m, n, T, 2, 0, True, lo, hi, 3, 1, seed=7, random_chain=0)                   # paper_results
    with pytest.raises(PpdeHipError, match=r"\[-1\].*paper_results"):
        ch.set_reversible(True)
    ch.set_reversible(False)                                                                 # (switching it off is no conflict)
    ch.close()
    # a letter outside the library at an open residue: no error at this level, and that residue never moves
    site = int(dl.open_sites(lib)[0])
    outside = next(k for k in range(20) if not (int(lib[site]) >> k) & 1)
    x0[:, site] = outside
    ch = Chains(m, n, T, 2, 0, False, lo, hi, 3, 1, seed=7, random_chain=0, trace=True)
    ch.set_library(lib)
    ch.set_reversible(True)
    ch.init(torch.as_tensor(x0).cuda())
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_reversible(True)
    with pytest.raises(PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_reversible(False)
    ch.run(T)
    ch.sync()
    res, tr, pk = ch.collect(), ch.trace(), ch.peek()
    assert (pk["idx"][:, site] == outside).all() and (res["best_idx"][:, site] == outside).all()
    assert (res["random_traj"][:, site] == outside).all()
    moved = (tr["flat"] // 20 == site) & (tr["flat"] >= 0)
    assert moved.any() and not tr["accepted"].astype(bool)[moved.any(1)].any()               # proposed there, always rejected
    assert tr["accepted"].any() and (pk["idx"] != x0).any()                                  # while the other residues move
    ch.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 8. sharding
def test_sharding_does_not_change_a_reversible_run(toy):
    c, lib, _ = toy
    m = hl.hip_model_of(c)
    T = 25

    def run(n_, off):
        ch = _chains(m, c, n_, T, 2, 3, 1, lib, lo=c["i0"], hi=c["i0"] + c["Lp"] - 1, chain_offset=off, random_chain=0 if off == 0 else -1)
        ch.run(T)
        r = ch.collect()
        ch.close()
        return r

    one, a, b = run(16, 0), run(7, 0), run(9, 7)
    for k in ("energy_history", "fitness_history"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 1), one[k]), k
    for k in ("best_idx", "best_energy", "best_fitness", "best_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]], 0), one[k]), k
    assert np.array_equal(a["random_traj"], one["random_traj"])
    assert (one["energy_history"][1:] != one["energy_history"][:-1]).any()
    m.close()


# ------------------------------------------------------------------------------------------------ 9. PPDE_PAS
def test_ppde_pas_runs_the_chains_a_caller_would_build_by_hand():
    """args.ppde_reversible through PPDE_PAS.run (no library given: all letters over [min_pos, max_pos], folded, chains over the
    full range) against the same run assembled from Chains: identical histories, best states and trajectory."""
    import argparse
    import contextlib
    import io
    import tempfile
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    import os
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        args = argparse.Namespace(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n,
                                  device="cuda:0", ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox",
                                  ppde_seed=seed, ppde_reversible=True)
        en = ProteinProductOfExperts(args)
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        np.random.seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            sampler = PPDE_PAS(args)
            best_x, best_e, best_f, e_hist, f_hist, rtraj = sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10)
        assert sampler.last_chains.reversible is True
        L = len(seq)
        assert np.array_equal(sampler.last_chains.library, dl.fold_range(dl.full_library(L), i0, i0 + Lp - 1))
        np.random.seed(5)
        ch = Chains(en.model, n, T, pas, nmut, False, 0, L - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_library(dl.fold_range(dl.full_library(L), i0, i0 + Lp - 1))
        ch.set_reversible(True)
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        res = ch.collect()
        ch.close()
        assert np.array_equal(e_hist, res["energy_history"]) and np.array_equal(f_hist, res["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), res["best_idx"]) and np.array_equal(best_e, res["best_energy"])
        assert np.array_equal(np.stack([r.argmax(-1) for r in rtraj]), res["random_traj"])
        assert (e_hist[1:] != e_hist[:-1]).any()
        outside = np.r_[0:i0, i0 + Lp:L]
        assert (res["best_idx"][:, outside] == res["best_idx"][0, outside]).all()

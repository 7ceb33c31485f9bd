"""The pair counts on the GPU (ppde_chains_set_pair_counts; k_record_pairs in ppde_amd/csrc/pairs.h): they equal, exactly, the
reference of the samples the recorder stored in the same run (helpers_pairs.pair_counts_of, the only reference) at every layout
edge, population and site list, from graphs and eagerly, in every mode and under both gradient policies, with a counts-only
recorder and with a recorder that follows a rung; nothing else of the run changes; the counted block follows the enumerated law;
the interfaces around them.

Everything but the law test is exact (array_equal, other results compared as bytes). The law test uses
tests/test_reversible_gpu.py's statistic, bound and case unchanged (helpers_library.chi_square, chi_square_bound; 34 degrees of
freedom). tests/test_pairs_cpu.py asserts that the start populations used here can see a transposed kernel."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_pairs as hp
import helpers_reversible as hr
import helpers_tempering as ht
from ppde_amd import library as dl
from ppde_amd import synthetic

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
RECORD_KEYS = ("idx", "energy", "fitness", "chain", "site_counts")
N, T_LONG, PAS, NMUT, SEED = 16, 130, 2, 3, 202           # 130 = one 100 segment, one 20 segment and 10 eager steps
BETAS = ht.REPLAY_BETAS
MODES = ("default", "library", "reversible", "tempering")
ALL = "all"                                               # (the `pairs` argument of _make: every residue; None: no pair counts)


def _same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _make(m, c, lib, mode, n, T, rng_mode=1, reuse=True, swap_every=1, recorder=None, pairs=None, x0=None, lo=None, hi=None, nmut=NMUT,
          betas=BETAS, init=True, **kw):
    from ppde_amd.sampler import Chains
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", SEED)
    lo = c["i0"] if lo is None else lo
    hi = c["i0"] + c["Lp"] - 1 if hi is None else hi
    ch = Chains(m, n, T, PAS, nmut, False, lo, hi, 3 if c.get("cnn") is not None else 1, rng_mode, reuse_grad=reuse, **kw)
    if mode != "default":
        ch.set_library(lib)
    if mode in ("reversible", "tempering"):
        ch.set_reversible(True)
    if mode == "tempering":
        ch.set_tempering(betas, swap_every)
    if recorder is not None:
        ch.set_recorder(**recorder)
    if pairs is not None:
        ch.set_pair_counts(None if isinstance(pairs, str) else pairs)
    if init:
        x0 = np.tile(c["wt"], (n, 1)) if x0 is None else x0
        ch.init(torch.as_tensor(x0).cuda())
    return ch


def _assert_pair_counts(counts, sites, rec, want_sites, label=""):
    """The counts against the reference of the stored samples, and the identities that tie them to the site counts."""
    idx = rec["idx"]
    rows, slots, L = idx.shape
    want_sites = np.arange(L, dtype=np.int32) if want_sites is None else np.asarray(want_sites, np.int32)
    S = want_sites.size
    assert sites.dtype == np.int32 and np.array_equal(sites, want_sites), label
    assert counts.dtype == np.uint64 and counts.shape == (S, 20, S, 20), label
    assert np.array_equal(counts, hp.pair_counts_of(idx, want_sites)), label
    M = counts.reshape(S * 20, S * 20)
    assert np.array_equal(M, M.T), label
    sc = rec["site_counts"][want_sites]
    assert np.array_equal(counts[np.arange(S), :, np.arange(S), :], np.stack([np.diag(v) for v in sc])), label
    assert (counts.sum((1, 3)) == rows * slots).all(), label
    assert np.array_equal(counts.sum(3), np.broadcast_to(sc[:, :, None], (S, 20, S))), label


@pytest.fixture(scope="module")
def toy():
    c, lib = hr.replay_model()
    m = hl.hip_model_of(c)
    yield c, lib, m
    m.close()


# ------------------------------------------------------------------------------------------------ 1. the reference, at the edges
@pytest.mark.parametrize("n", hp.POPULATIONS)
@pytest.mark.parametrize("L,i0,Lp", hp.GEOMETRIES)
def test_counts_equal_the_reference_of_the_stored_samples(L, i0, Lp, n):
    """Potts-only geometries with state rows of 5 to 61 dwords (a nonzero byte offset of residue 0 among them), populations on both
    sides of a wave and of a workgroup's pass over the slots, every residue and scattered lists with ragged last tiles; all-letters
    library over the full range, reversible, mutation cap off, T = 6, every = 1, from uniformly random letters."""
    c = hl.potts_case(L, i0, Lp, seed=31)
    m = hl.hip_model_of(c)
    T = 6
    x0 = hp.start_population(L, n)
    first = None
    for sites in hp.site_lists(L):
        label = f"L={L} n={n} S={'all' if sites is None else len(sites)}"
        ch = _make(m, c, dl.full_library(L), "reversible", n, T, recorder=dict(every=1), pairs=ALL if sites is None else sites, x0=x0,
                   lo=0, hi=L - 1, nmut=0, seed=500 + n, random_chain=-1)
        ch.run(T)
        rec = ch.recorded()
        counts, got_sites = ch.pair_counts()
        ch.close()
        assert rec["rows"] == T and rec["idx"].shape == (T, n, L), label
        _assert_pair_counts(counts, got_sites, rec, sites, label)
        if first is None:
            first = rec
            assert (rec["idx"][-1] != x0).any() or n == 1, "no chain moved: the run added nothing to the start population"
        assert np.array_equal(rec["idx"], first["idx"]), label                                # the site list changes no sample
    m.close()


# ------------------------------------------------------------------------------------------------ 2. the contention extreme
def test_identical_chains_put_every_slot_into_one_bin():
    """L = 8 with one open residue, all chains from the wild type, burn_in = 0: every frozen pair of residues has exactly one
    nonzero bin, rows * slots, which every lane of every wave adds to."""
    c = ht.one_site_case(8, 6, 1, 4)
    m = hl.hip_model_of(c)
    L, site, T = 8, 4, 6
    frozen = np.setdiff1d(np.arange(L), [site])
    for n in (64, 257, 1024):
        ch = _make(m, c, c["allowed"], "reversible", n, T, recorder=dict(every=1, burn_in=0), pairs=ALL, lo=0, hi=L - 1, nmut=0,
                   seed=77 + n, random_chain=-1)
        ch.run(T)
        rec = ch.recorded()
        counts, sites = ch.pair_counts()
        ch.close()
        _assert_pair_counts(counts, sites, rec, None, f"n={n}")
        for i in frozen:
            for j in frozen:
                block = counts[i, :, j, :]
                assert block[c["wt"][i], c["wt"][j]] == T * n and np.count_nonzero(block) == 1, (n, i, j)
        assert np.count_nonzero(counts[site, :, site, :]) > 1                                # the open residue moved
    m.close()


# ------------------------------------------------------------------------------------------------ 3. segments, modes, policies
_ALONE = {}


def _run(toy, mode, reuse, recorder, pairs, swap_every=1, T=T_LONG, n=N, **kw):
    c, lib, m = toy
    ch = _make(m, c, lib, mode, n, T, 1, reuse, swap_every, recorder=recorder, pairs=pairs, trace=True, **kw)
    ch.run(T)
    gs = ch.graph_stats()
    assert (gs["replayed_steps"], gs["eager_steps"]) == ((T // 20) * 20, T % 20)              # graphs and eager issue both ran
    out = dict(rec=ch.recorded(), res=ch.collect(), tr=ch.trace(), pairs=ch.pair_counts() if pairs is not None else None)
    ch.close()
    return out


def _alone(toy, mode, reuse, burn_in, every, swap_every=1, rung=None):
    """The same run with the recorder alone: computed once per configuration."""
    key = (mode, reuse, burn_in, every, swap_every if mode == "tempering" else None, rung)
    if key not in _ALONE:
        _ALONE[key] = _run(toy, mode, reuse, dict(every=every, burn_in=burn_in, rung=rung), None, swap_every)
    return _ALONE[key]


def _assert_nothing_else_changed(out, alone, label):
    for k in RESULT_KEYS:
        assert _same_bytes(out["res"][k], alone["res"][k]), (label, k)
    for k in TRACE_KEYS:
        assert _same_bytes(out["tr"][k], alone["tr"][k]), (label, k)
    for k in RECORD_KEYS:
        assert _same_bytes(out["rec"][k], alone["rec"][k]), (label, k)
    assert out["rec"]["rows"] == alone["rec"]["rows"], label


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_counts_accumulate_across_graph_segments_and_eager_steps(toy, mode, reuse):
    """TOY24, Potts + CNN, 16 chains, T = 130 on the device RNG (default mode: mutation cap 3, resets included), recorders
    (burn_in, every) = (0, 1) and (3, 4): the counts are the reference of the recorded rows, and every other array of the run is
    that of the run with the recorder alone, bit for bit."""
    c, _, _ = toy
    for burn_in, every in ((0, 1), (3, 4)):
        label = f"{mode} reuse={reuse} burn_in={burn_in} every={every}"
        out = _run(toy, mode, reuse, dict(every=every, burn_in=burn_in), ALL)
        alone = _alone(toy, mode, reuse, burn_in, every)
        assert out["rec"]["rows"] == (T_LONG - burn_in) // every
        _assert_pair_counts(*out["pairs"], out["rec"], None, label)
        _assert_nothing_else_changed(out, alone, label)
        assert (out["rec"]["idx"] != c["wt"][None, None]).any(), "no chain ever left the wild type"


def test_counts_on_caller_supplied_noise(toy):
    """rng_mode 0: every iteration its own eager launch sequence."""
    import ppde_oracle as orc
    c, lib, m = toy
    T = 12
    gen = torch.Generator().manual_seed(77)
    noise = [orc.draw_noise_torch(N, c["L"] * 20, PAS, generator=gen) for _ in range(T)]
    for mode in ("default", "reversible"):
        ch = _make(m, c, lib, mode, N, T, 0, recorder=dict(every=2, burn_in=1), pairs=ALL)
        for U, q, u in noise:
            ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))
        rec = ch.recorded()
        assert rec["rows"] == 5
        _assert_pair_counts(*ch.pair_counts(), rec, None, mode)
        ch.close()


# ------------------------------------------------------------------------------------------------ 4. counts-only recorder
def test_counts_only_recorder_has_the_same_pair_counts(toy):
    c, _, _ = toy
    sites = hp.scattered_sites(c["L"], 9, 5)
    for mode in ("default", "reversible"):
        keep = _run(toy, mode, True, dict(every=3, burn_in=2, keep_samples=True), sites)
        only = _run(toy, mode, True, dict(every=3, burn_in=2, keep_samples=False), sites)
        assert only["rec"]["idx"] is None and keep["rec"]["rows"] == only["rec"]["rows"] == 42
        _assert_pair_counts(*keep["pairs"], keep["rec"], sites, mode)
        assert np.array_equal(only["pairs"][0], keep["pairs"][0]) and np.array_equal(only["pairs"][1], keep["pairs"][1])
        assert np.array_equal(only["rec"]["site_counts"], keep["rec"]["site_counts"])


# ------------------------------------------------------------------------------------------------ 5. with a ladder
@pytest.mark.parametrize("swap_every", [1, 5])
def test_counts_follow_the_recorded_rung(toy, swap_every):
    c, _, _ = toy
    R = len(BETAS)
    sites = hp.scattered_sites(c["L"], 5, 11)
    seen = []
    for rung in (0, R - 1):
        for pairs in (ALL, sites):
            label = f"swap_every={swap_every} rung={rung}"
            out = _run(toy, "tempering", True, dict(every=1, burn_in=0, rung=rung), pairs, swap_every)
            rec = out["rec"]
            assert rec["chain"].shape == (T_LONG, N // R)
            assert (rec["chain"] != (np.arange(N // R) * R + rung)[None]).any(), "no accepted swap moved the slot: nothing was followed"
            _assert_pair_counts(*out["pairs"], rec, None if pairs is ALL else sites, label)
            _assert_nothing_else_changed(out, _alone(toy, "tempering", True, 0, 1, swap_every, rung), label)
        seen.append(out["pairs"][0])
    assert not np.array_equal(seen[0], seen[1])                                              # the two rungs hold different samples


# ------------------------------------------------------------------------------------------------ 6. a second start
def test_a_second_init_counts_from_zero(toy):
    c, lib, m = toy
    T = 25
    ch = _make(m, c, lib, "reversible", N, 2 * T, recorder=dict(every=1), pairs=ALL)
    zero, _ = ch.pair_counts()
    assert not zero.any()
    ch.run(T)
    first, _ = ch.pair_counts()
    rec = ch.recorded()
    _assert_pair_counts(first, np.arange(c["L"], dtype=np.int32), rec, None)
    ch.run(T)
    assert ch.pair_counts()[0].sum() == 2 * first.sum()                                      # the read covers all rows so far
    ch.init(torch.as_tensor(np.tile(c["wt"], (N, 1))).cuda())
    assert not ch.pair_counts()[0].any() and not ch.recorded()["site_counts"].any()
    ch.run(T)
    assert np.array_equal(ch.pair_counts()[0], first)                                        # the same run from zero, not on top
    ch.close()


# ------------------------------------------------------------------------------------------------ 7. the law
def test_law_of_the_counted_block():
    """law_case(), 2^16 reversible chains, a counts-only recorder with burn_in = 63, every = 1, T = 64, sites = [2, 3]: the
    off-diagonal block is the histogram of the population over the 35 states after 64 iterations, held against exp(E)/Z with the
    statistic and bound of tests/test_reversible_gpu.py (34 degrees of freedom); bins outside the library are exactly 0."""
    from test_reversible_gpu import _law
    c, K, states, index, e, inside = _law("two residues, 7 and 5 letters, paths of 1-3 moves")
    pi = hr.target_law(e, inside)
    m = hl.hip_model_of(c)
    n, T = 1 << 16, 64
    ch = _make(m, c, c["allowed"], "reversible", n, T, recorder=dict(every=1, burn_in=63, keep_samples=False), pairs=[2, 3], lo=0,
               hi=c["L"] - 1, nmut=c["nmut"], seed=6047, random_chain=-1)
    ch.run(T)
    assert ch.recorder_shape() == (1, 1, n)
    counts, sites = ch.pair_counts()
    site_counts = ch.recorded()["site_counts"]
    ch.close()
    m.close()
    assert sites.tolist() == [2, 3] and counts.shape == (2, 20, 2, 20)
    block = counts[0, :, 1, :]
    assert block.sum() == n and np.array_equal(block.T, counts[1, :, 0, :])
    assert np.array_equal(block.sum(1), site_counts[2]) and np.array_equal(block.sum(0), site_counts[3])
    ok = dl.as_bool(c["allowed"])
    assert not block[~(ok[2][:, None] & ok[3][None, :])].any()                                # outside the library: exactly 0
    S = states.shape[0]
    assert S == 35 and int((ok[2][:, None] & ok[3][None, :]).sum()) == 35
    hist = np.zeros(S, np.float64)
    for (a, b), s in index.items():
        hist[s] = block[a, b]
    assert hist.sum() == n
    chi2, df = hl.chi_square(hist, n * pi)
    print(f"pair-count law, block (2, 3) after 64 iterations: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df == 34
    assert chi2 < hl.chi_square_bound(df), (chi2, df)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_pair_count_refusals(toy):
    from ppde_amd import _hip
    from ppde_amd.sampler import Chains
    c, lib, m = toy
    lo, hi, L = c["i0"], c["i0"] + c["Lp"] - 1, c["L"]
    n, T = 8, 30
    bad = pytest.raises
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no recorder was set"):
        ch.set_pair_counts()
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no pair counts were set"):
        ch.pair_counts()
    ch.clear_pair_counts()                                                                   # clearing nothing is fine
    ch.set_recorder(every=1)
    for sites, what in (([-1, 2], "outside the sequence"), ([0, L], "outside the sequence"), ([1, 1], "strictly increasing"),
                        ([0, 5, 4], "strictly increasing"), (list(range(L)) + [L], "n_sites must be in 0..L")):
        with bad(_hip.PpdeHipError, match=rf"\[-1\].*{what}"):
            ch.set_pair_counts(sites)
    arr = (ctypes.c_int32 * 2)(0, 1)
    for n_sites, ptr, what in ((-1, None, "n_sites must be in 0..L"), (2, None, "needs a site list"), (0, arr, "site list with n_sites = 0")):
        cfg = _hip.PairConfig(n_sites=n_sites, sites=ptr)
        with bad(_hip.PpdeHipError, match=rf"\[-1\].*{what}"):
            _hip.check(ch.lib.ppde_chains_set_pair_counts(ch.handle, ctypes.byref(cfg)))
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no pair counts were set"):                     # every refusal left the object unchanged
        ch.pair_counts()
    ch.set_pair_counts([L - 1])
    ch.set_pair_counts([0, 3, L - 1])                                                        # replaced
    S = ctypes.c_int32()
    _hip.check(ch.lib.ppde_chains_pair_counts_shape(ch.handle, ctypes.byref(S), None))
    assert S.value == 3
    with bad(_hip.PpdeHipError, match=r"\[-1\].*clear the pair counts first"):
        ch.set_recorder(None)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*clear the pair counts first"):
        ch.set_recorder(every=2)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*chains not initialised"):
        ch.pair_counts()
    ch.clear_pair_counts()
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no pair counts were set"):                     # the read after clear
        ch.pair_counts()
    ch.set_recorder(every=2)                                                                 # without them the recorder may change again
    ch.set_recorder(None)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no recorder was set"):
        ch.set_pair_counts()
    ch.set_recorder(every=2)
    ch.set_pair_counts()
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.set_pair_counts([0, 1])
    with bad(_hip.PpdeHipError, match=r"\[-1\].*before ppde_chains_init"):
        ch.clear_pair_counts()
    ch.run(T)
    counts, sites = ch.pair_counts()
    _assert_pair_counts(counts, sites, ch.recorded(), None)
    assert ch.lib.ppde_chains_pair_counts_read(ch.handle, None) == 0                          # NULL: synchronises only
    ch.close()
    ch = Chains(m, n, T, 2, 3, False, lo, hi, 3, 1, seed=7)                                   # a run without them reads nothing
    ch.set_recorder(every=1)
    ch.init(torch.as_tensor(np.tile(c["wt"], (n, 1))).cuda())
    ch.run(5)
    with bad(_hip.PpdeHipError, match=r"\[-1\].*no pair counts were set"):
        ch.pair_counts()
    ch.close()


# ------------------------------------------------------------------------------------------------ 9. sharding, PPDE_PAS, driver
def test_sharding_sums_to_the_unsharded_counts(toy):
    c, lib, m = toy
    T, R = 25, len(BETAS)
    sites = hp.scattered_sites(c["L"], 8, 3)

    def run(mode, n_, off, rung):
        ch = _make(m, c, lib, mode, n_, T, recorder=dict(every=2, burn_in=1, rung=rung), pairs=sites, chain_offset=off, random_chain=-1,
                   seed=99)
        ch.run(T)
        out = ch.recorded(), ch.pair_counts()[0]
        ch.close()
        return out

    for mode, rung in (("default", None), ("reversible", None), ("tempering", 0), ("tempering", R - 1)):
        (one, p_one), (a, p_a), (b, p_b) = run(mode, 16, 0, rung), run(mode, 8, 0, rung), run(mode, 8, 8, rung)
        assert np.array_equal(np.concatenate([a["idx"], b["idx"]], 1), one["idx"]), mode
        assert np.array_equal(p_a + p_b, p_one), mode
        assert np.array_equal(p_one, hp.pair_counts_of(one["idx"], sites)), mode


def test_ppde_pas_and_the_driver_hand_the_pair_counts_out():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    L = len(seq)
    n, T, pas, nmut, seed = 8, 30, 2, 3, 4242
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        base = dict(energy_lamda=5.0, unsupervised_expert="potts", protein_weights=root, protein="TOY24", n_chains=n, device="cuda:0",
                    ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False, ppde_rng="philox", ppde_seed=seed,
                    ppde_sample_every=4, ppde_sample_burn_in=2)
        en = ProteinProductOfExperts(argparse.Namespace(**base))
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        wt = en.model.onehot_to_idx(x0).cpu().numpy()[0]
        lib = dl.build_library(wt, (i0, i0 + Lp - 1), sites=[i0 + 1, i0 + 2, i0 + 5])

        def run(**extra):
            np.random.seed(5)
            with contextlib.redirect_stdout(io.StringIO()):
                sampler = PPDE_PAS(argparse.Namespace(**base, **extra))
                out = sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10)
            return sampler.samples, out

        plain, out_plain = run()
        assert plain["pair_counts"] is None and plain["pair_sites"] is None                   # off: both None
        for extra, want in ((dict(ppde_sample_pairs="all"), np.arange(L)),
                            (dict(ppde_sample_pairs="open"), np.arange(i0, i0 + Lp)),
                            (dict(ppde_sample_pairs="open", ppde_library=lib), np.array([i0 + 1, i0 + 2, i0 + 5])),
                            (dict(ppde_sample_pairs="open", ppde_library=lib, ppde_reversible=True), np.array([i0 + 1, i0 + 2, i0 + 5])),
                            (dict(ppde_sample_pairs=f"0,{i0}-{i0 + 2},{L - 1}"), np.array([0, i0, i0 + 1, i0 + 2, L - 1])),
                            (dict(ppde_sample_pairs=[1, L - 2]), np.array([1, L - 2])),
                            (dict(ppde_sample_pairs="all", ppde_sample_counts_only=True), np.arange(L))):
            got, out = run(**extra)
            assert len(out) == 6                                                             # the returned tuple does not change
            assert got["pair_sites"].dtype == np.int32 and np.array_equal(got["pair_sites"], want), extra
            assert got["pair_counts"].shape == (len(want), 20, len(want), 20) and got["pair_counts"].dtype == np.uint64
            if "ppde_library" not in extra:
                assert all(_same_bytes(a, b) for a, b in zip(out[1:5], out_plain[1:5])), extra
                assert np.array_equal(got["site_counts"], plain["site_counts"])
            if got["idx"] is not None:
                assert np.array_equal(got["pair_counts"], hp.pair_counts_of(got["idx"], want)), extra
            else:
                assert np.array_equal(got["pair_counts"], hp.pair_counts_of(plain["idx"], want)), extra
        # the driver: the two files beside the recorder's, equal to the reference of samples.npy
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_pairs", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        common = ["--protein_weights", root, "--protein", "TOY24", "--results_path", res, "--device", "cuda:0",
                  "--disable_MSA_transformer_scoring", "--n_chains", "12", "--n_iters", "40", "--seed", "3", "--log_every", "25",
                  "--nmut_threshold", "4", "--ppde_rng", "philox", "--ppde_sample_every", "5", "--ppde_sample_burn_in", "10"]
        for sig, flags, want in (("pairs_all", ["--ppde_sample_pairs", "all"], np.arange(L)),
                                 ("pairs_spec", ["--ppde_sample_pairs", f"{i0}-{i0 + 3},{L - 1}"], np.array([i0, i0 + 1, i0 + 2, i0 + 3, L - 1])),
                                 ("pairs_open", ["--ppde_sample_pairs", "open", "--ppde_sites", f"{i0 + 1},{i0 + 4}"], np.array([i0 + 1, i0 + 4]))):
            args = drv.build_parser().parse_args(common + ["--run_signature", sig] + flags)
            args.ppde_reuse_grad = True
            with contextlib.redirect_stdout(io.StringIO()):
                out = drv.main(args)
            names = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
            assert {"pair_counts.npy", "pair_sites.npy", "site_counts.npy", "samples.npy"} <= names
            pc, ps, sm = (np.load(os.path.join(out, f)) for f in ("pair_counts.npy", "pair_sites.npy", "samples.npy"))
            assert sm.shape == (6, 12, L) and ps.dtype == np.int32 and np.array_equal(ps, want), sig
            assert pc.dtype == np.uint64 and np.array_equal(pc, hp.pair_counts_of(sm, want)), sig
        args = drv.build_parser().parse_args(common + ["--run_signature", "no_pairs"])
        args.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(args)
        assert not {"pair_counts.npy", "pair_sites.npy"} & {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}

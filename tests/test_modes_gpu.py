"""Library, reversible, tempering, recorder and pair-count runs on the expert sets no other module runs them on: the supervised
expert alone (which = 2), the transformer expert (5, 6, 7) and the full gradient (7 | 8). These take gwhich != which (rows without
lamda * d fit / dx under an energy with lamda * fit), the transformer term of slot_energy / finish_energy under beta, beta * g over
a row that sums the transformer's gradient, e = fit in the swap rule, and the eager iteration loop (no graph behind a transformer).

The reference is the CPU iteration of each mode (tests/helpers_library.py, helpers_reversible.py, helpers_tempering.py) on
`helpers_modes.DeviceEnergy`: the device's own experts, read through ppde_energy_grad. What is left to differ is the chain kernels'
fp32 arithmetic, held to the project's standards: draws, accept bits, best states, random_traj, rung histories and swap counters
exact; log_acc 2e-4; energy / fitness histories 2e-5 max(1, |e|) / 5e-6 max(1, |f|). A chain may leave the reference only at a
near-tie of the reference's own decision (race gap <= 1e-5, |log_acc - log u| <= 2e-4; with a ladder its ensemble leaves with it):
at most one chain (ensemble) per run and two such runs in the module. tests/test_modes_cpu.py shows what this comparison rejects.

Model: tests/test_transformer_gpu.py's _model at TOY24 length (L = 24, Potts window (4, 16)), 2 layers, 128 / 4 heads, ffn 256,
three seeded CNNs, lamda = 2; 16 chains, T = 20, pas 2, nmut 3. The seeded CNNs' fitness spans 0.03 only, so a which = 2 ladder
refuses a swap about once in a hundred decisions: the Philox key of its swap_every 1 cell is one that refuses a swap and shows a
swap decided on fit * lamda (helpers_modes.PHILOX_SEEDS); the law case on scaled CNNs carries that check for the rest."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_library as hl
import helpers_modes as hm
import helpers_pairs as hp
import helpers_reversible as hr
import helpers_tempering as ht
from helpers import device_noise
from ppde_amd import library as dl
from ppde_amd import synthetic
from test_hip_parity import observed

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
PARTED_RUNS = []                     # tags of the runs in which a chain left the reference at a validated near-tie


def _model(L=hm.TOY["L"], win=hm.TOY["win"], cnn_gain=1.0):
    from ppde_amd.energy import HipModel
    wt, J, h, cnn, st = hm.toy_parts(L, win)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, win[0])
    m.set_cnn(hm.scaled_cnn(cnn, cnn_gain))
    m.set_transformer(st, hm.TOY["heads"])
    m.set_lamda(hm.LAMDA)
    return m, wt


@pytest.fixture(scope="module")
def toy():
    m, wt = _model()
    yield m, wt, hm.window_library(wt, hm.TOY["win"])
    m.close()


def _chains(m, wt, which, mode, lib, win, rng_mode, n=hm.N, T=hm.T, nmut=hm.NMUT, x0=None, full_range=False, recorder=None, pairs=None,
            betas="mode", swap_every=None, **kw):
    from ppde_amd.sampler import Chains
    use_lib, rev, mode_betas, mode_swap = hm.mode_settings(mode, lib)
    betas = mode_betas if isinstance(betas, str) else betas
    kw.setdefault("random_chain", 0)
    kw.setdefault("seed", hm.philox_seed(which, mode))
    lo, hi = (0, len(wt) - 1) if full_range else (win[0], win[0] + win[1] - 1)
    ch = Chains(m, n, T, hm.PAS, nmut, False, lo, hi, which, rng_mode, **kw)
    if use_lib is not None:
        ch.set_library(use_lib)
    if rev:
        ch.set_reversible(True)
    if betas is not None:
        ch.set_tempering(betas, mode_swap if swap_every is None else swap_every)
        if recorder is not None and "rung" not in recorder:
            recorder = dict(recorder, rung=0)
    if recorder is not None:
        ch.set_recorder(**recorder)
        if pairs is not None:
            ch.set_pair_counts(pairs)
    ch.init(torch.as_tensor(np.tile(wt, (n, 1)) if x0 is None else x0).cuda())
    return ch


def _feed(ch, noise):
    for U, q, u in noise:
        ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))


def _read(ch, tempering):
    temp = None
    if tempering:
        st = ch.tempering_state()
        temp = dict(hist=ch.tempering_history(), rung=st["rung"], beta=st["beta"], swap_attempts=st["swap_attempts"],
                    swap_accepts=st["swap_accepts"])
    return dict(tr=ch.trace(), res=ch.collect(), temp=temp)


def _same_bits(a, b, label):
    for k in RESULT_KEYS:
        assert np.array_equal(a["res"][k], b["res"][k]), (label, k)
    for k in TRACE_KEYS:
        assert np.array_equal(a["tr"][k], b["tr"][k]), (label, k)
    if a["temp"] is not None:
        for k in a["temp"]:
            assert np.array_equal(a["temp"][k], b["temp"][k]), (label, k)


def _cell(m, wt, lib, win, which, mode, rng_mode, n=hm.N, T=hm.T, tag_extra=""):
    """One cell of the matrix: reuse and re-evaluate runs, identical to each other, against the reference on DeviceEnergy."""
    L = len(wt)
    tempering = mode.startswith("temp")
    seed = hm.philox_seed(which, mode)
    noise = hm.torch_noise(which, mode, n, L, T) if rng_mode == 0 else None
    runs = []
    for reuse in (True, False):
        ch = _chains(m, wt, which, mode, lib, win, rng_mode, n=n, T=T, trace=True, reuse_grad=reuse)
        if rng_mode == 0:
            _feed(ch, noise)
        else:
            ch.run(T)
            if noise is None:
                noise = device_noise(ch, T, hm.PAS)
        runs.append(_read(ch, tempering))
        ch.close()
    _same_bits(runs[0], runs[1], f"{which}:{mode}: reuse against re-evaluate")
    ref = hm.reference_run(mode, hm.DeviceEnergy(m, which), wt, lib, noise, win, seed, n=n)
    tag = f"{which}:{mode}:rng{rng_mode}{tag_extra}"
    out = hm.compare_replay(tag, runs[0], ref, noise, R=len(hm.BETAS) if tempering else 1, record=observed,
                            lib=hm.mode_settings(mode, lib)[0])
    print(f"[modes] {tag}: parted {out['parted']}, log_acc {out['log_acc']:.3f}, energy {out['energy']:.3f}, fitness {out['fitness']:.3f} "
          f"of the tolerance, histories bit-equal: {out['bit_equal']}")
    groups = {b // len(hm.BETAS) for b in out["parted"]} if tempering else set(out["parted"])
    assert len(groups) <= 1, f"{tag}: more than one chain (ensemble) left the reference: {out['notes']}"
    if groups:
        PARTED_RUNS.append(tag)
    assert len(PARTED_RUNS) <= 2, f"runs with a parted chain: {PARTED_RUNS}"
    acc = runs[0]["tr"]["accepted"]
    assert acc.any() and not acc.all()
    return runs[0], ref, noise


# ------------------------------------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("mode", hm.MODES)
@pytest.mark.parametrize("which", hm.WHICH)
def test_device_rng_replay(toy, which, mode):
    m, wt, lib = toy
    dev, ref, noise = _cell(m, wt, lib, hm.TOY["win"], which, mode, 1)
    if mode.startswith("temp"):
        assert dev["temp"]["swap_accepts"].sum() > 0
        if (which, mode) in hm.PHILOX_SEEDS:
            # the key of this cell was picked so that a swap is refused and a swap decided on fit * lamda shows (test_modes_cpu.py)
            assert dev["temp"]["swap_accepts"].sum() < dev["temp"]["swap_attempts"].sum()
            with hm.swap_on_scaled_energy(m.lamda):
                bad = hm.reference_run(mode, hm.DeviceEnergy(m, which), wt, lib, noise, hm.TOY["win"], hm.philox_seed(which, mode))
            assert not np.array_equal(bad["rung_history"], dev["temp"]["hist"])


@pytest.mark.parametrize("mode", hm.MODES)
@pytest.mark.parametrize("which", [2, 7])
def test_torch_noise_replay(toy, which, mode):
    m, wt, lib = toy
    _cell(m, wt, lib, hm.TOY["win"], which, mode, 0)


@pytest.mark.parametrize("mode", ["rev_lib", "temp_lib"])
@pytest.mark.parametrize("L,win", hm.LARGE)
def test_two_and_three_groups_per_thread(L, win, mode):
    """which = 7 at L = 104 (window (23, 76)) and L = 237 (window (0, 237): ring Potts, chunked CNN, 256-row attention), where the
    library's words share the LDS with two and three groups per thread."""
    assert (L * 5 + 511) // 512 == {104: 2, 237: 3}[L]
    m, wt = _model(L, win)
    lib = hm.window_library(wt, win)
    _cell(m, wt, lib, win, 7, mode, 1, n=hm.N_LARGE, T=hm.T_LARGE, tag_extra=f":L{L}")
    m.close()


# ------------------------------------------------------------------------------------------------ 2. identities without a reference
@pytest.mark.parametrize("which", [2, 7])
def test_identities(toy, which):
    """A ladder (1.0,) is the reversible run, and the library of all letters is no library in reversible mode, bit for bit."""
    m, wt, lib = toy
    win = hm.TOY["win"]
    full = dl.full_library(len(wt))                      # (not folded to the window: the range mask stays what it is without a library)
    for reuse in (True, False):
        out = []
        for mode, use, betas in (("rev", lib, None), ("rev", lib, (1.0,)), ("rev_lib", full, None)):
            ch = _chains(m, wt, which, mode, use, win, 1, trace=True, reuse_grad=reuse, betas=betas, swap_every=1, seed=4100 + which)
            ch.run(hm.T)
            r = _read(ch, False)
            out.append(r)
            ch.close()
        assert out[0]["tr"]["accepted"].any() and not out[0]["tr"]["accepted"].all()
        _same_bits(out[0], out[1], f"which {which} reuse {reuse}: ladder (1.0,)")
        _same_bits(out[0], out[2], f"which {which} reuse {reuse}: full library")


# ------------------------------------------------------------------------------------------------ 3. recorder and pair counts
@pytest.mark.parametrize("mode,rung", [("rev_lib", None), ("temp_lib", 0), ("temp_lib", len(hm.BETAS) - 1)])
@pytest.mark.parametrize("which", [2, 7])
def test_recorder_and_pair_counts_behind_the_experts(toy, which, mode, rung):
    """tests/test_recorder_gpu.py's method: a recorded row is the peek of a stepped twin without a recorder after that iteration;
    the site counts are the counts of those rows, the pair counts helpers_pairs' reference on them; nothing else changes."""
    m, wt, lib = toy
    win, L, T, every, burn_in = hm.TOY["win"], len(wt), hm.T, 3, 2
    sites = hp.scattered_sites(L, 5, 17)
    twin = _chains(m, wt, which, mode, lib, win, 1, trace=True)
    peeks = [twin.peek()]
    for _ in range(T):
        twin.run(1)
        peeks.append(twin.peek())
    want = _read(twin, mode.startswith("temp"))
    twin.close()
    ch = _chains(m, wt, which, mode, lib, win, 1, trace=True, recorder=dict(every=every, burn_in=burn_in, rung=rung), pairs=sites)
    ch.run(T)
    got, rec = _read(ch, mode.startswith("temp")), ch.recorded()
    counts, got_sites = ch.pair_counts()
    ch.close()
    _same_bits(got, want, f"which {which} {mode}: the recorder changes the run")
    rows = (T - burn_in) // every
    assert rec["rows"] == rows == 6 and rec["idx"].shape == (rows, hm.N // len(hm.BETAS) if rung is not None else hm.N, L)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for s in range(rows):
        t = burn_in + (s + 1) * every
        pk, chain = peeks[t], rec["chain"][s]
        if rung is not None:
            assert (want["temp"]["hist"][t][chain] == rung).all()
        assert np.array_equal(rec["idx"][s], pk["idx"][chain]), s
        assert np.array_equal(bits(rec["energy"][s]), bits(pk["energy"][chain])) and np.array_equal(bits(rec["fitness"][s]), bits(pk["fitness"][chain])), s
    site_counts = np.stack([np.bincount(rec["idx"][:, :, l].ravel(), minlength=20) for l in range(L)]).astype(np.uint64)
    assert np.array_equal(rec["site_counts"], site_counts)
    assert np.array_equal(got_sites, sites) and np.array_equal(counts, hp.pair_counts_of(rec["idx"], sites))
    assert (rec["idx"] != wt[None, None]).any()


# ------------------------------------------------------------------------------------------------ 4. the law
def _cells_against(label, counts_of, expected, n):
    chi2, df = hl.chi_square(counts_of.astype(np.float64), n * expected)
    print(f"[modes law] {label}: chi2 {chi2:.1f} on {df} degrees of freedom (bound {hl.chi_square_bound(df):.1f})")
    assert df >= 10, "the case must spread over enough cells to test anything"
    assert chi2 < hl.chi_square_bound(df), (label, chi2, df)


def test_law_of_a_reversible_run_on_all_experts(toy):
    """which = 7, reversible, one open residue with 20 letters, 65 536 chains from the wild type: the population after T = 1, 2, 12
    against the kernel enumerated on the device's own energies and gradients (no fp16 bias enters the statistic)."""
    m, wt, _ = toy
    L, n = len(wt), 1 << 16
    allowed = hm.one_site_library(wt, hm.LAW_SITE)
    K, states, index, _, _ = hr.exact_reversible_kernel(hm.DeviceEnergy(m, 7), wt, allowed, hm.PAS, 0, L - 1, 0)
    start = index[(int(wt[hm.LAW_SITE]),)]
    for T in (1, 2, 12):
        ch = _chains(m, wt, 7, "rev_lib", allowed, hm.TOY["win"], 1, n=n, T=T, nmut=0, full_range=True, random_chain=-1, seed=6100 + T)
        ch.run(T)
        ch.sync()
        idx = ch.peek()["idx"]
        ch.close()
        cells, forbidden = hl.state_cells(idx, allowed, index, wt)
        assert forbidden == 0
        _cells_against(f"which 7 reversible T={T}", np.bincount(cells, minlength=K.shape[0]), hm.population_law(K, start, T), n)


def test_law_of_a_ladder_on_the_supervised_expert():
    """which = 2, ladder (1, 1/2) with a swap event behind every iteration, 65 536 chains = 32 768 ensembles, one open residue with 8
    letters, the CNNs' output layer scaled by 256 (fitness spans 1.4 over the states instead of 0.005, so that the swap and
    accept decisions decide something: tests/test_modes_cpu.py), started on the states of lowest and highest energy."""
    m, wt = _model(cnn_gain=hm.LAW_GAIN_2)
    L, n_ens, R = len(wt), 1 << 15, 2
    case = dict(wt=wt, allowed=hm.one_site_library(wt, hm.LAW_SITE, hm.LAW_LETTERS_2), L=L, nmut=0)
    Ks, states, index, E, _ = hm.kernels_of(hm.DeviceEnergy(m, 2), case, ht.BETAS_A, hm.PAS)
    S = states.shape[0]
    start = hm.law_start_2(E)
    x0 = np.tile(np.stack([states[s].numpy().astype(np.uint8) for s in start]), (n_ens, 1))
    for T in (1, 2, 12):
        expected = ht.joint_law(T, Ks, E, ht.BETAS_A, 1, start[0] * S + start[1])
        ch = _chains(m, wt, 2, "temp_lib", case["allowed"], hm.TOY["win"], 1, n=n_ens * R, T=T, nmut=0, x0=x0, full_range=True,
                     betas=ht.BETAS_A, swap_every=1, random_chain=-1, seed=6200 + T)
        ch.run(T)
        ch.sync()
        idx, st = ch.peek()["idx"], ch.tempering_state()
        ch.close()
        cells, forbidden = ht.joint_cells(idx, st["rung"], R, case["allowed"], index, states[start[0]].numpy(), S)
        assert forbidden == 0
        _cells_against(f"which 2 ladder T={T} (swaps {st['swap_accepts'].sum()} / {st['swap_attempts'].sum()})",
                       np.bincount(cells, minlength=S ** R), expected, n_ens)
    m.close()


# ------------------------------------------------------------------------------------------------ 5. PPDE_PAS and the driver
def test_ppde_pas_and_the_driver_with_every_feature_behind_the_transformer():
    import argparse
    import contextlib
    import glob
    import importlib.util
    import io
    import os
    import tempfile
    from ppde_amd.energy import ProteinProductOfExperts
    from ppde_amd.nets import AugmentedLinearRegression
    from ppde_amd.sampler import Chains, PPDE_PAS
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    L = len(seq)
    n, T, pas, nmut, seed = 8, 20, 2, 3, 4242
    betas = (1.0, 0.5, 0.25, 0.125)
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as res:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        synthetic.write_esm2_checkpoint(os.path.join(res, "checkpoints", "esm2_t30_150M_UR50D.pt"), 2, 128, 4, 256, seed=2)
        from ppde_amd.encoding import seqs_to_idx
        lib = hl.seeded_library(seqs_to_idx([seq])[0], i0, i0 + Lp - 1, seed=41)
        args = argparse.Namespace(energy_lamda=2.0, unsupervised_expert="potts+transformer", protein_weights=root, protein="TOY24",
                                  n_chains=n, device="cuda:0", hub_dir=res, ppde_pas_length=pas, nmut_threshold=nmut, paper_results=False,
                                  ppde_rng="philox", ppde_seed=seed, ppde_reversible=True, ppde_betas=betas, ppde_swap_every=2,
                                  ppde_library=lib, ppde_sample_every=3, ppde_sample_burn_in=2, ppde_sample_pairs="open")
        en = ProteinProductOfExperts(args)
        assert en.which == 7
        alr = AugmentedLinearRegression(os.path.join(root, "TOY24"))
        x0 = en.wt_onehot.repeat(n, 1, 1)
        np.random.seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            sampler = PPDE_PAS(args)
            best_x, best_e, best_f, e_hist, f_hist, rtraj = sampler.run(x0, T, en, i0, i0 + Lp - 1, alr, log_every=10)
        np.random.seed(5)
        words = dl.fold_range(dl.as_words(lib, L), i0, i0 + Lp - 1)
        ch = Chains(en.model, n, T, pas, nmut, False, 0, L - 1, en.which, 1, random_chain=np.random.randint(0, n), seed=seed)
        ch.set_library(words)
        ch.set_reversible(True)
        ch.set_tempering(betas, 2)
        ch.set_recorder(3, 2, 0)
        ch.set_pair_counts(dl.open_sites(words).astype(np.int32))
        ch.init(en.model.onehot_to_idx(x0))
        ch.run(T)
        r, st, hist, rec = ch.collect(), ch.tempering_state(), ch.tempering_history(), ch.recorded()
        pc, ps = ch.pair_counts()
        ch.close()
        assert np.array_equal(e_hist, r["energy_history"]) and np.array_equal(f_hist, r["fitness_history"])
        assert np.array_equal(best_x.argmax(-1).cpu().numpy(), r["best_idx"]) and np.array_equal(best_e, r["best_energy"])
        assert np.array_equal(np.stack([x.argmax(-1) for x in rtraj]), r["random_traj"])
        assert np.array_equal(sampler.tempering["rung_history"], hist) and np.array_equal(sampler.tempering["swap_accepts"], st["swap_accepts"])
        got = sampler.samples
        assert got["rows"] == rec["rows"] == 6
        for k in ("idx", "energy", "fitness", "chain", "site_counts"):
            assert np.array_equal(got[k], rec[k]), k
        assert np.array_equal(got["pair_counts"], pc) and np.array_equal(got["pair_sites"], ps) and ps.size == int((words != 0).sum())
        assert np.array_equal(pc, hp.pair_counts_of(rec["idx"], ps))
        assert (e_hist[1:] != e_hist[:-1]).any()
        # the driver with the same flags: its sample, pair-count and rung files
        spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_modes", os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py"))
        drv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(drv)
        argv = ["--protein_weights", root, "--protein", "TOY24", "--results_path", res, "--hub_dir", res, "--device", "cuda:0",
                "--disable_MSA_transformer_scoring", "--sampler", "PPDE", "--unsupervised_expert", "potts+transformer", "--n_chains", "8",
                "--n_iters", "20", "--seed", "3", "--log_every", "10", "--energy_lamda", "2", "--nmut_threshold", "3", "--ppde_rng", "philox",
                "--ppde_reversible", "--ppde_betas", "1,0.5,0.25,0.125", "--ppde_swap_every", "2", "--ppde_sites", f"{i0 + 2}-{i0 + 9}",
                "--ppde_sample_every", "3", "--ppde_sample_burn_in", "2", "--ppde_sample_pairs", "open", "--run_signature", "modes"]
        a = drv.build_parser().parse_args(argv)
        a.ppde_reuse_grad = True
        with contextlib.redirect_stdout(io.StringIO()):
            out = drv.main(a)
        shapes = {"samples.npy": (6, 2, L), "sample_energy.npy": (6, 2), "sample_fitness.npy": (6, 2), "sample_chain.npy": (6, 2),
                  "site_counts.npy": (L, 20), "pair_counts.npy": (8, 20, 8, 20), "pair_sites.npy": (8,), "rung_history.npy": (21, 8),
                  "swap_attempts.npy": (2, 3), "swap_accepts.npy": (2, 3)}
        have = {os.path.basename(f) for f in glob.glob(os.path.join(out, "*"))}
        assert set(shapes) <= have, sorted(set(shapes) - have)
        for f, shape in shapes.items():
            assert np.load(os.path.join(out, f)).shape == shape, f
        sm = np.load(os.path.join(out, "samples.npy"))
        sites = np.load(os.path.join(out, "pair_sites.npy"))
        assert np.array_equal(sites, np.arange(i0 + 2, i0 + 10))
        assert np.array_equal(np.load(os.path.join(out, "pair_counts.npy")), hp.pair_counts_of(sm, sites))
        eh, rh = np.load(os.path.join(out, "energy_history.npy")), np.load(os.path.join(out, "rung_history.npy"))
        chain = np.load(os.path.join(out, "sample_chain.npy"))
        for s in range(6):
            t = 2 + 3 * (s + 1)
            assert (rh[t][chain[s]] == 0).all() and np.array_equal(np.load(os.path.join(out, "sample_energy.npy"))[s], eh[t][chain[s]])

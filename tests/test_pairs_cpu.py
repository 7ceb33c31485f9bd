"""The pair counts without a GPU: the reference helper on hand-made populations, what PPDE_PAS refuses and how it reads
ppde_sample_pairs before any device work, the driver's flag, the host side of the C ABI as a stand-alone program under
AddressSanitizer (tests/hostcheck/pairs.cpp), and the power condition of tests/test_pairs_gpu.py: on its seeded start populations the
reference differs from itself with the letters of an off-diagonal block exchanged, and from itself with the two sites exchanged
without their letters, so a kernel (or an unpacking) that transposes either would be seen."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_library as hl
import helpers_pairs as hp


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_on_hand_made_populations():
    # two rows of three slots over five residues
    idx = np.array([[[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [5, 1, 7, 3, 19]],
                    [[5, 6, 7, 8, 9], [0, 6, 2, 8, 4], [19, 19, 19, 19, 19]]], np.uint8)
    sites = [0, 2, 4]
    c = hp.pair_counts_of(idx, sites)
    assert c.shape == (3, 20, 3, 20) and c.dtype == np.uint64
    want = np.zeros_like(c)
    for row in idx.reshape(-1, 5):
        for i, si in enumerate(sites):
            for j, sj in enumerate(sites):
                want[i, row[si], j, row[sj]] += 1
    assert np.array_equal(c, want)
    assert c[0, 0, 1, 2] == 3 and c[0, 5, 1, 7] == 2 and c[0, 19, 2, 19] == 1 and c[0, 5, 2, 19] == 1 and c[0, 0, 1, 7] == 0
    site_counts = np.stack([np.bincount(idx[:, :, l].ravel(), minlength=20) for l in range(5)]).astype(np.uint64)
    M = c.reshape(60, 60)
    assert np.array_equal(M, M.T)                                                            # symmetric as a matrix
    for i, si in enumerate(sites):
        assert np.array_equal(c[i, :, i, :], np.diag(site_counts[si]))                       # diagonal blocks
        for j in range(3):
            assert c[i, :, j, :].sum() == 6                                                  # every block: rows * slots
            assert np.array_equal(c[i, :, j, :].sum(1), site_counts[si])                     # the marginal is the one-point count
    # the Gram matrix of the one-hot rows
    X = np.zeros((6, 60), np.int64)
    for r, row in enumerate(idx.reshape(-1, 5)):
        X[r, np.arange(3) * 20 + row[sites]] = 1
    assert np.array_equal(M.astype(np.int64), X.T @ X)
    # all residues, a single sample, a single site
    assert np.array_equal(hp.pair_counts_of(idx, np.arange(5))[np.ix_([0, 2, 4], range(20), [0, 2, 4], range(20))], c)
    one = hp.pair_counts_of(idx[:1, :1], [3])
    assert one.shape == (1, 20, 1, 20) and one.sum() == 1 and one[0, 3, 0, 3] == 1
    # more samples than one pass of the bincount holds
    big = np.random.default_rng(3).integers(0, 20, (3, 700, 90)).astype(np.uint8)
    cb = hp.pair_counts_of(big, np.arange(90))
    assert (cb.sum((1, 3)) == 2100).all() and np.array_equal(cb.reshape(1800, 1800), cb.reshape(1800, 1800).T)


def test_site_lists_of_the_gpu_test():
    for L, _, _ in hp.GEOMETRIES:
        lists = hp.site_lists(L)
        assert lists[0] is None
        assert [len(s) for s in lists[1:]] == [S for S in hp.SITE_COUNTS if S <= L]
        for s in lists[1:]:
            assert (np.diff(s) > 0).all() and s[-1] == L - 1 and (len(s) == 1 or s[0] == 0)
    assert [len(s) for s in hp.site_lists(8)[1:]] == [1, 3, 4, 5, 8]


# ------------------------------------------------------------------------------------------------ the power of the GPU test
def test_the_gpu_test_can_see_a_transposed_kernel():
    for L, _, _ in hp.GEOMETRIES:
        for n in hp.POPULATIONS:
            x0 = hp.start_population(L, n)
            assert x0.shape == (n, L) and x0.max() < 20
            for sites in hp.site_lists(L):
                s = np.arange(L) if sites is None else sites
                if len(s) < 2:
                    continue
                c = hp.pair_counts_of(x0[None], s)
                off = ~np.eye(len(s), dtype=bool)
                letters_swapped = c.transpose(0, 3, 2, 1)                                     # [i, b, j, a]
                sites_swapped = c.transpose(2, 1, 0, 3)                                      # [j, a, i, b]
                assert (letters_swapped != c).any((1, 3))[off].any(), (L, n, len(s))
                assert (sites_swapped != c).any((1, 3))[off].any(), (L, n, len(s))
                assert np.array_equal(c.transpose(2, 3, 0, 1), c)                            # both at once is the symmetry itself


# ------------------------------------------------------------------------------------------------ PPDE_PAS
class _NoDevice:
    which = 1

    def __getattr__(self, name):
        raise AssertionError(f"PPDE_PAS touched the model ({name}) before refusing")


def _args(**kw):
    return argparse.Namespace(ppde_pas_length=2, nmut_threshold=0, paper_results=False, ppde_rng="philox", seed=1, **kw)


def test_ppde_pas_reads_and_refuses_the_pair_spec_before_any_device_work():
    from ppde_amd.encoding import idx_to_onehot
    from ppde_amd.sampler import PPDE_PAS, check_pair_spec, pair_sites_of
    assert PPDE_PAS(_args()).sample_pairs is None                                             # off by default
    for off in (None, "", "  "):
        assert PPDE_PAS(_args(ppde_sample_every=2, ppde_sample_pairs=off)).sample_pairs is None
        assert PPDE_PAS(_args(ppde_sample_pairs=off)).sample_pairs is None                    # off needs no recorder
    for spec, want in (("all", "all"), ("ALL", "all"), ("open", "open"), (" Open ", "open"), ("2-4,6", "2-4,6"), ([0, 3, 5], (0, 3, 5)),
                       (np.array([1, 2]), (1, 2)), ((4,), (4,))):
        assert PPDE_PAS(_args(ppde_sample_every=2, ppde_sample_pairs=spec)).sample_pairs == want
    for bad, what in ((dict(ppde_sample_pairs="all"), "needs ppde_sample_every"),
                      (dict(ppde_sample_pairs=[1, 2]), "needs ppde_sample_every"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs="3-1"), "runs backwards"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs="1,,2"), "empty token"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs="some"), "cannot read site token"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs="-1"), "ppde_sample_pairs"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=[2, 2]), "strictly increasing"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=[3, 1]), "strictly increasing"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=[-1, 1]), "strictly increasing"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=[]), "at least one"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=[1.5]), "whole number"),
                      (dict(ppde_sample_every=2, ppde_sample_pairs=7), "expected 'all'")):
        with pytest.raises(ValueError, match=what):
            PPDE_PAS(_args(**bad))
    # what a spec selects in a sequence of 7 whose sampler moves in 1..5
    lib = np.zeros(7, np.uint32)
    lib[[2, 3]] = 0xFFFFF
    assert pair_sites_of("all", 7, 1, 5) is None
    assert pair_sites_of("open", 7, 1, 5).tolist() == [1, 2, 3, 4, 5] and pair_sites_of("open", 7, 1, 5).dtype == np.int32
    assert pair_sites_of("open", 7, 1, 5, lib).tolist() == [2, 3]
    assert pair_sites_of("5,0-2", 7, 1, 5).tolist() == [0, 1, 2, 5]
    assert pair_sites_of((0, 6), 7, 1, 5).tolist() == [0, 6]
    assert check_pair_spec("open") == "open"
    # beyond the sequence: refused by run() before the model is touched
    c = hl.law_case()
    x0 = torch.from_numpy(idx_to_onehot(np.tile(c["wt"], (6, 1)))).float()
    ef = argparse.Namespace(model=_NoDevice(), which=1)
    for spec in ("0-7", "7", [0, 7]):
        with pytest.raises(ValueError, match="outside the sequence 0..6"):
            PPDE_PAS(_args(ppde_sample_every=1, ppde_sample_pairs=spec)).run(x0, 5, ef, 0, c["L"] - 1, None)
    # a spec that fits goes on to the device (here: to the stand-in, which says so)
    for spec in ("all", "open", "0-6", [0, 6]):
        with pytest.raises(AssertionError, match="touched the model"):
            PPDE_PAS(_args(ppde_sample_every=1, ppde_sample_pairs=spec)).run(x0, 5, ef, 0, c["L"] - 1, None)


def test_cli_flag_parses_into_the_sampler_argument():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "directed_evolution.py")
    spec = importlib.util.spec_from_file_location("directed_evolution_cli_pairs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--ppde_sample_every", "10", "--ppde_sample_pairs", "8-20,33"])
    assert a.ppde_sample_pairs == "8-20,33"
    assert mod.build_parser().parse_args([]).ppde_sample_pairs is None
    from ppde_amd.sampler import PPDE_PAS
    assert PPDE_PAS(argparse.Namespace(**{**vars(a), "ppde_library": None})).sample_pairs == "8-20,33"
    assert "29 MB at 96 sites" in re.sub(r"\s+", " ", mod.build_parser().format_help())


# ------------------------------------------------------------------------------------------------ the host layer
def test_host_layer_of_the_pair_counts_under_address_sanitizer():
    """tests/hostcheck/pairs.cpp: a stand-alone C++ driver (its own main) over the host side of the C ABI and the mock runtime of
    tests/hostcheck/, compiled with AddressSanitizer + LeakSanitizer: every refusal, then a valid set, shape, init, run, read,
    clear and destroy, then the walk once per fallible runtime call with that call failing. Any leak or out-of-bounds access fails
    the run."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "build_and_run.sh")
    r = subprocess.run(["bash", script, "pairs", "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"hostcheck pairs ok: (\d+) fallible runtime calls per walk, (\d+) injected failures handled", r.stdout)
    assert m and int(m.group(1)) > 100 and m.group(1) == m.group(2), r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

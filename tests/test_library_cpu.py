"""Design libraries without a GPU: the masked reference of the GPU tests against the oracle it is made of, the parser and
builders of ppde_amd/library.py, and the new entry of the C ABI in header, binding and shared library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppde_oracle as orc
import helpers_library as hl
from ppde_amd import library as dl
from ppde_amd.encoding import ALPHABET

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = np.iinfo(np.int32).max


# ------------------------------------------------------------------------------------------------ the masked reference
def test_all_letters_library_is_the_oracle_bit_for_bit():
    c = hl.toy24()
    en = hl.oracle_energy_of(c)
    n, T, pas, L = 8, 6, 2, c["L"]
    torch.manual_seed(17)
    noise = [orc.draw_noise_torch(n, L * 20, pas) for _ in range(T)]
    x0 = np.tile(c["wt"].astype(np.int64), (n, 1))
    args = (en, x0, c["wt"], lambda t: noise[t], T, c["i0"], c["i0"] + c["Lp"] - 1, pas, 3, False)
    ref = orc.run(*args, trace=True)
    got = hl.masked_run(dl.full_library(L), *args, trace=True)
    for k in ("best_idx", "best_energy", "best_fitness", "energy_history", "fitness_history", "states", "accepted", "final_idx"):
        assert torch.equal(ref[k], got[k]), k
    for a, b in zip(ref["traces"], got["traces"]):
        for k in ("flat", "log_acc", "logp_fwd", "logp_rev"):
            assert torch.equal(a[k], b[k]), k
    assert orc.forward_logits.__module__ == "ppde_oracle" and orc.categorical_probs.__module__ == "ppde_oracle"   # restored


@pytest.fixture(scope="module")
def law():
    c = hl.law_case()
    en = hl.oracle_energy_of(dict(c, cnn=None, lamda=0.0))
    K, states, index = hl.exact_library_kernel(en, c["wt"], c["allowed"], 2, 0, c["L"] - 1)
    return c, en, K, states, index


def test_enumerated_kernel_is_a_distribution_over_allowed_states_only(law):
    c, en, K, states, index = law
    assert K.shape == (35, 35) and (K >= 0).all()
    assert np.abs(K.sum(1) - 1.0).max() <= 1e-6                  # no leak column: nothing is lost to entries outside the library
    # and the masked proposal holds EXACTLY 0 on every forbidden entry, from every state, along paths of three moves
    forbid = ~dl.as_bool(c["allowed"]).reshape(-1)
    S, L = states.shape
    gen = torch.Generator().manual_seed(3)
    U, q, u = orc.draw_noise_torch(S, L * 20, 2, generator=gen)
    with hl.masked_oracle(c["allowed"]):
        out = orc.pas_iteration(en, states, states, torch.as_tensor(c["wt"].astype(np.int64)), torch.full((S,), 3), q[:1].repeat(3, 1, 1), u,
                                0, L - 1, INT_MAX, keep_probs=True)
    p = out["p_fwd"].numpy()
    assert (p[:, :, forbid] == 0.0).all() and (p[:, :, ~forbid] > 0.0).all()
    assert np.abs(p.sum(-1) - 1.0).max() <= 1e-6
    assert not forbid[out["flat"].numpy()].any()
    # the same with the range mask doing part of the work (window 2..3): entries masked ONLY by the range keep the floor,
    # but here every such entry is forbidden as well, so the proposal is the same
    with hl.masked_oracle(c["allowed"]):
        out2 = orc.pas_iteration(en, states, states, torch.as_tensor(c["wt"].astype(np.int64)), torch.full((S,), 3), q[:1].repeat(3, 1, 1), u,
                                 2, 3, INT_MAX, keep_probs=True)
    assert torch.equal(out["p_fwd"], out2["p_fwd"])


def test_range_masked_entries_keep_the_floor_under_a_library():
    """Entries masked only by the position range (or the cap) keep the reference's 2^-23 floor: the library removes what IT forbids."""
    c = hl.law_case()
    en = hl.oracle_energy_of(dict(c, cnn=None, lamda=0.0))
    L = c["L"]
    lib = c["allowed"].copy()
    lib[5] = dl.ALL_LETTERS                                      # open in the library, outside the range 2..3
    x = torch.as_tensor(c["wt"].astype(np.int64)).reshape(1, -1)
    q = torch.ones(1, 1, L * 20)
    with hl.masked_oracle(lib):
        out = orc.pas_iteration(en, x, x, x[0], torch.ones(1, dtype=torch.int64), q, torch.full((1,), 0.5), 2, 3, INT_MAX, keep_probs=True)
    p = out["p_fwd"][0, 0].reshape(L, 20).numpy()
    assert (p[5] > 0).all() and (p[5] < 2e-7).all()             # floor / sum
    assert (p[[0, 1, 4, 6]] == 0).all()


@pytest.mark.parametrize("two_level", [False, True])
def test_masked_oracle_sampler_follows_the_enumerated_kernel(law, two_level):
    """40 000 chains of the masked reference on torch's CPU noise, one iteration (paths of 1-3 moves) from the wild type and from a
    second state (chosen from K alone), against rows of K: the flat race and the two-level draw of the device RNG (oracle race_sample)."""
    c, en, K, states, index = law
    S, L, n, pas = states.shape[0], c["L"], 40000, 2
    gen = torch.Generator().manual_seed(5)
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    # the second start state: the one (other than the wild type) whose row of K spreads over the most cells above the merge floor
    spread = ((n * K) >= 8.0).sum(1)
    spread[wt_row] = -1
    for start in (wt_row, int(np.argmax(spread))):
        U, q, u = orc.draw_noise_torch(n, L + 20 if two_level else L * 20, pas, generator=gen)
        x = states[start].repeat(n, 1)
        with hl.masked_oracle(c["allowed"]):
            out = orc.pas_iteration(en, x, x, torch.as_tensor(c["wt"].astype(np.int64)), U.reshape(-1), q, u, 0, L - 1, INT_MAX)
        cells, forbidden = hl.state_cells(out["idx"].numpy(), c["allowed"], index, states[start].numpy())
        assert forbidden == 0
        chi2, df = hl.chi_square(np.bincount(cells, minlength=S).astype(np.float64), n * K[start])
        print(f"two_level={two_level} start={start}: chi2 {chi2:.1f} on {df} degrees of freedom")
        assert df >= 10 and chi2 < hl.chi_square_bound(df), (start, chi2, df)


def test_law_geometry_spreads_over_enough_cells():
    """The GPU law test's own condition, checked on the reference alone: at pas 1 from the wild type with 2^16 chains, the
    enumerated kernel's powers hold at least 11 cells above the merge floor of 8 (df >= 10)."""
    c = hl.law_case()
    en = hl.oracle_energy_of(dict(c, cnn=None, lamda=0.0))
    K, states, index = hl.exact_library_kernel(en, c["wt"], c["allowed"], 1, 0, c["L"] - 1)
    wt_row = index[(int(c["wt"][2]), int(c["wt"][3]))]
    for T in (1, 2, 12):
        E = (1 << 16) * np.linalg.matrix_power(K, T)[wt_row]
        assert (E >= 8.0).sum() >= 11, (T, int((E >= 8.0).sum()))


# ------------------------------------------------------------------------------------------------ parser, builders, rules
def test_site_lists():
    assert dl.parse_sites("8-20,33,40-44", 96) == list(range(8, 21)) + [33] + list(range(40, 45))
    assert dl.parse_sites(" 3 , 1-2,2", 10) == [1, 2, 3]
    for spec, token in (("8-20,x3", "x3"), ("5-2", "5-2"), ("1,,2", "empty"), ("0-96", "0-96"), ("3-4-5", "3-4-5"), ("-1", "-1")):
        with pytest.raises(ValueError, match=re.escape(token)):
            dl.parse_sites(spec, 96)


def test_library_file_and_letters(tmp_path):
    text = "# campaign 7\n8 ACD  # three letters\n\n10 acdefghiklmnpqrstvwy\n12 W\n"
    e = dl.parse_library_text(text, 24)
    assert e == {8: 0b111, 10: dl.ALL_LETTERS, 12: 1 << ALPHABET.index("W")}
    p = tmp_path / "lib.txt"
    p.write_text(text)
    assert dl.parse_library_file(p, 24) == e
    for bad, token in (("8 AXC", "'X'"), ("8", "'8'"), ("q ACD", "'q'"), ("24 A", "'24'"), ("8 A\n8 C", "'8'"), ("8 A C", "8 A C")):
        with pytest.raises(ValueError, match=re.escape(token)):
            dl.parse_library_text(bad, 24)
    assert dl.bits_to_letters(dl.letters_to_bits("YCA")) == "ACY"
    with pytest.raises(ValueError, match="'B'"):
        dl.letters_to_bits("AB")


def test_builders_keep_the_wild_type_and_fold_the_range():
    c = hl.toy24()
    wt, L, lo, hi = c["wt"], c["L"], c["i0"], c["i0"] + c["Lp"] - 1
    # default: every site of the window, all letters
    lib = dl.build_library(wt, (lo, hi))
    assert (lib[lo:hi + 1] == dl.ALL_LETTERS).all() and (lib[:lo] == 0).all() and (lib[hi + 1:] == 0).all()
    assert len(dl.open_sites(lib)) == c["Lp"] and abs(dl.log10_size(lib) - c["Lp"] * np.log10(20)) < 1e-9
    # sites + exclude: the wild-type letter of an open site survives the exclusion
    sites = dl.parse_sites("5-7,12", L)
    excl = ALPHABET[int(wt[5])] + "C"
    lib = dl.build_library(wt, (lo, hi), sites=sites, exclude=excl)
    assert list(dl.open_sites(lib)) == [5, 6, 7, 12]
    b = dl.as_bool(lib)
    assert b[5, wt[5]] and all(b[s, wt[s]] for s in sites)
    for s in sites:
        for ch in excl:
            k = ALPHABET.index(ch)
            assert b[s, k] == (k == wt[s])
    assert "4 open sites" in dl.summary(lib) and f"{dl.log10_size(lib):.3f}" in dl.summary(lib)
    # a library file: exactly the listed sites, the wild type added, the exclusion on top
    lib = dl.build_library(wt, (lo, hi), exclude="C", entries={6: dl.letters_to_bits("CD"), 9: dl.letters_to_bits("W"), 10: 0})
    assert list(dl.open_sites(lib)) == [6, 9]
    assert dl.bits_to_letters(lib[6]) == "".join(sorted(set("D" + ALPHABET[int(wt[6])]), key=ALPHABET.index))
    # outside the window / the sequence, and nothing open
    with pytest.raises(ValueError, match="site 2 lies outside the window"):
        dl.build_library(wt, (lo, hi), sites=[2, 5])
    with pytest.raises(ValueError, match="no open site"):
        dl.build_library(wt, (lo, hi), sites=[])
    # both forms of a mask, and the range folded into the library
    full = dl.full_library(L)
    assert np.array_equal(dl.as_words(dl.as_bool(lib)), lib) and dl.as_bool(full).all()
    f = dl.fold_range(full, lo, hi)
    assert (f[lo:hi + 1] == dl.ALL_LETTERS).all() and not f[:lo].any() and not f[hi + 1:].any() and full.all()
    with pytest.raises(ValueError, match="bit >= 20"):
        dl.as_words(np.array([1 << 20], np.uint32))
    with pytest.raises(ValueError, match="24"):
        dl.as_words(full[:5], L)


def test_driver_flags_build_the_library(tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ppde_amd_directed_evolution_lib", os.path.join(REPO, "scripts", "directed_evolution.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    c = hl.toy24()
    wt, lo, hi = c["wt"], c["i0"], c["i0"] + c["Lp"] - 1
    parse = lambda *a: drv.build_parser().parse_args(list(a))
    assert drv.design_library_from_flags(parse(), wt, lo, hi) is None                      # no flag: no library, today's run
    lib = drv.design_library_from_flags(parse("--ppde_sites", "5-7,12", "--ppde_exclude", "CM"), wt, lo, hi)
    assert list(dl.open_sites(lib)) == [5, 6, 7, 12]
    out = capsys.readouterr().out
    assert re.search(r"design library: 4 open sites, log10\(size\) = \d+\.\d+", out)
    lib = drv.design_library_from_flags(parse("--ppde_exclude", "C"), wt, lo, hi)
    assert len(dl.open_sites(lib)) == c["Lp"]
    p = tmp_path / "lib.txt"
    p.write_text("6 CD\n9 W\n")
    lib = drv.design_library_from_flags(parse("--ppde_library", str(p), "--ppde_sites", "5", "--ppde_exclude", "C"), wt, lo, hi)
    assert list(dl.open_sites(lib)) == [6, 9]                                                # the file replaces --ppde_sites
    with pytest.raises(ValueError, match="'7-x'"):
        drv.design_library_from_flags(parse("--ppde_sites", "5,7-x"), wt, lo, hi)
    with pytest.raises(ValueError, match="'Z'"):
        drv.design_library_from_flags(parse("--ppde_exclude", "CZ"), wt, lo, hi)
    help_text = drv.build_parser().format_help()
    assert "wild-type" in help_text and "--ppde_sites" in help_text and "--ppde_library" in help_text


# ------------------------------------------------------------------------------------------------ header / binding / library
def test_set_library_is_declared_bound_and_exported():
    from ppde_amd import _hip, build
    build.build()
    hdr = open(os.path.join(REPO, "include", "ppde_hip.h")).read()
    assert re.search(r"^int\s+ppde_chains_set_library\s*\(\s*ppde_chains\*\s*c,\s*const uint32_t\*\s*allowed_host", hdr, flags=re.M)
    assert "ppde.py:60-63" in hdr and "ppde.py:98-110" in hdr and "utils.py:106-111" in hdr
    assert "ppde_chains_set_library" in _hip.SIGNATURES
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "ppde_chains_set_library")
    assert re.search(r"#define\s+PPDE_ABI_VERSION\s+1\b", hdr)
    from ppde_amd.sampler import Chains
    assert callable(getattr(Chains, "set_library"))

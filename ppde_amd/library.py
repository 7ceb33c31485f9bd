"""Design libraries: the letters the sampler may PROPOSE at each residue (include/ppde_hip.h, ppde_chains_set_library).

A library is `allowed[L]`, one uint32 word per residue of the full sequence: bit k set = letter ALPHABET[k] may be proposed
there, word 0 = the residue is frozen. Positions are 0-based indices into the full sequence, the index space of the
`min_pos max_pos` line a run prints. The wild-type letter of an open residue always stays in the library (the mutation cap's
only move is the revert to the wild type). A library constrains moves only: initial states need not lie inside it.
"""
import math
import os

import numpy as np

from .encoding import ALPHABET

A = len(ALPHABET)
ALL_LETTERS = (1 << A) - 1


def letters_to_bits(letters):
    """'ACD' -> bit mask; ValueError names a letter outside the alphabet."""
    bits = 0
    for ch in letters:
        k = ALPHABET.find(ch.upper()) if ch.strip() else -1
        if k < 0:
            raise ValueError(f"design library: {ch!r} in {letters!r} is not one of the {A} letters {ALPHABET}")
        bits |= 1 << k
    return bits


def bits_to_letters(bits):
    return "".join(ALPHABET[k] for k in range(A) if (int(bits) >> k) & 1)


def parse_sites(spec, L):
    """'8-20,33,40-44' -> sorted list of 0-based positions (ranges inclusive). ValueError names the offending token."""
    out = set()
    for tok in str(spec).split(","):
        t = tok.strip()
        if not t:
            if str(spec).strip() == "":
                continue
            raise ValueError(f"design library: empty token in site list {spec!r}")
        parts = t.split("-")
        try:
            if len(parts) == 1:
                lo = hi = int(parts[0])
            elif len(parts) == 2:
                lo, hi = int(parts[0]), int(parts[1])
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"design library: cannot read site token {t!r} (expected '<pos>' or '<first>-<last>')") from None
        if lo > hi:
            raise ValueError(f"design library: site token {t!r} runs backwards")
        if lo < 0 or hi >= L:
            raise ValueError(f"design library: site token {t!r} lies outside the sequence 0..{L - 1}")
        out.update(range(lo, hi + 1))
    return sorted(out)


def parse_library_text(text, L):
    """Lines '<pos> <letters>', '#' starts a comment, blank lines ignored -> {pos: bits}. Unlisted positions are frozen."""
    entries = {}
    for no, raw in enumerate(str(text).splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        f = line.split()
        if len(f) != 2:
            raise ValueError(f"design library line {no}: expected '<pos> <letters>', got {line!r}")
        try:
            pos = int(f[0])
        except ValueError:
            raise ValueError(f"design library line {no}: cannot read position {f[0]!r}") from None
        if pos < 0 or pos >= L:
            raise ValueError(f"design library line {no}: position {f[0]!r} lies outside the sequence 0..{L - 1}")
        if pos in entries:
            raise ValueError(f"design library line {no}: position {f[0]!r} is listed twice")
        entries[pos] = letters_to_bits(f[1])
    return entries


def parse_library_file(path, L):
    with open(os.fspath(path)) as fh:
        return parse_library_text(fh.read(), L)


def full_library(L):
    """All twenty letters everywhere: the bits of a run without a library."""
    return np.full(int(L), ALL_LETTERS, np.uint32)


def fold_range(allowed, min_pos, max_pos):
    """Freeze every residue outside [min_pos, max_pos] (a copy): a library run then relies on no leaky range mask."""
    out = np.array(as_words(allowed), np.uint32, copy=True)
    out[:int(min_pos)] = 0
    out[int(max_pos) + 1:] = 0
    return out


def build_library(wt_idx, window=None, sites=None, exclude="", entries=None):
    """uint32 [L] from the driver's three inputs.

    wt_idx   wild-type letters [L] (indices into ALPHABET)
    window   (min_pos, max_pos) the sampler may move in; None = the whole sequence. A site or entry outside it is an error.
    sites    positions opened with all letters (None = every site of the window); ignored when `entries` is given
    exclude  letters removed at every open site
    entries  {pos: bits} from a library file: exactly these sites are open, with these letters
    The wild-type letter of an open site is always kept, whatever `exclude` or the entry says."""
    wt = np.asarray(wt_idx).astype(np.int64).reshape(-1)
    L = wt.shape[0]
    lo, hi = (0, L - 1) if window is None else (int(window[0]), int(window[1]))
    if not (0 <= lo <= hi < L):
        raise ValueError(f"design library: bad window [{lo}, {hi}] for a sequence of {L}")
    drop = letters_to_bits(exclude or "")
    if entries is not None:
        opened = {int(p): int(b) for p, b in entries.items()}
    else:
        opened = {p: ALL_LETTERS for p in (range(lo, hi + 1) if sites is None else sites)}
    out = np.zeros(L, np.uint32)
    for p, bits in opened.items():
        if p < 0 or p >= L:
            raise ValueError(f"design library: site {p} lies outside the sequence 0..{L - 1}")
        if p < lo or p > hi:
            raise ValueError(f"design library: site {p} lies outside the window {lo}..{hi} the sampler moves in")
        if bits >> A:
            raise ValueError(f"design library: site {p} has a letter index >= {A}")
        if bits == 0:
            continue                                        # listed without letters: frozen
        out[p] = (bits & ~drop) | (1 << int(wt[p]))
    if not out.any():
        raise ValueError("design library: no open site")
    return out


def check_population(allowed, idx):
    """ValueError if a state of idx [n, L] holds a letter outside the library at an OPEN residue. Reversible mode refuses such a
    population: the residue could never move (the move back to that letter is forbidden, so every path through it is rejected)."""
    ok = as_bool(allowed)
    idx = np.asarray(idx).astype(np.int64)
    opened = np.flatnonzero(ok.any(1))
    bad = ~ok[opened[None, :], idx[:, opened]]
    if bad.any():
        b, j = np.argwhere(bad)[0]
        raise ValueError(f"design library: chain {int(b)} starts with letter {ALPHABET[int(idx[b, opened[j]])]} at open residue "
                         f"{int(opened[j])}, which the library does not hold; in reversible mode that residue could never move")


def as_words(mask, L=None):
    """uint32 [L] from uint32 [L] or bool [L, 20]."""
    m = np.asarray(mask)
    if m.ndim == 2:
        if m.shape[1] != A or m.dtype != np.bool_:
            raise ValueError(f"design library: a 2-d mask must be bool [L, {A}], got {m.dtype} {m.shape}")
        words = (m.astype(np.uint32) << np.arange(A, dtype=np.uint32)).sum(1).astype(np.uint32)
    elif m.ndim == 1 and m.dtype.kind in "ui":
        if (m.astype(np.int64) < 0).any() or (m.astype(np.int64) >> A).any():
            raise ValueError(f"design library: a word has a bit >= {A} set")
        words = m.astype(np.uint32)
    else:
        raise ValueError(f"design library: expected uint32 [L] or bool [L, {A}], got {m.dtype} {m.shape}")
    if L is not None and words.shape[0] != int(L):
        raise ValueError(f"design library: {words.shape[0]} residues, the sequence has {int(L)}")
    return np.ascontiguousarray(words)


def as_bool(mask):
    """bool [L, 20] view of a library: [l, k] = letter k may be proposed at residue l."""
    w = as_words(mask)
    return ((w[:, None] >> np.arange(A, dtype=np.uint32)[None, :]) & 1).astype(bool)


def open_sites(mask):
    return np.flatnonzero(as_words(mask))


def log10_size(mask):
    """log10 of the number of sequences the library spans: sum over open sites of log10(letters)."""
    n = as_bool(mask).sum(1)
    return float(sum(math.log10(int(v)) for v in n if v > 0))


def summary(mask):
    """The driver's line: open sites and log10 of the library's size."""
    return f"design library: {len(open_sites(mask))} open sites, log10(size) = {log10_size(mask):.3f}"

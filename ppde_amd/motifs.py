"""Forbidden sequence patterns (include/ppde_hip.h, ppde_chains_set_forbidden_patterns): the text form, the rule in plain numpy, and
the device scan of candidate lists.

A pattern is a run of 1..8 elements, each a set of letters as a 20-bit word (bit k = letter ALPHABET[k], the design library's
convention). In text: a letter stands for itself, `x` for any letter, `[ST]` for a set, `{P}` for a complement, and `(n)` behind an
element repeats it: `N{P}[ST]`, `NG`, `K(4)`. A state matches pattern m at start p when p + len_m <= L and x[p + j] lies in element
j for every j. With allow_native the (pattern, start) pairs at which the wild type matches are exempt. A state is free when no
active (pattern, start) matches it.
"""
import ctypes as C

import numpy as np

from .encoding import ALPHABET

A = len(ALPHABET)
ALL_LETTERS = (1 << A) - 1
MAX_PATTERNS, MAX_LEN = 32, 8

PRESETS = {
    "n_glycosylation": "N{P}[ST]",
    "deamidation": "N[GS]",
    "isomerisation": "D[GS]",
}


class Patterns:
    """M patterns: elements uint32 [M, 8] (0 behind each length), lengths int32 [M], text (one string per pattern)."""

    def __init__(self, elements, lengths, text=None):
        self.elements = np.ascontiguousarray(np.asarray(elements, dtype=np.uint32).reshape(-1, MAX_LEN))
        self.lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        if self.elements.shape[0] != self.lengths.size:
            raise ValueError("forbidden patterns: elements and lengths disagree on the number of patterns")
        self.text = list(text) if text is not None else [element_text(self.elements[m], self.lengths[m]) for m in range(len(self))]

    def __len__(self):
        return int(self.lengths.size)


def element_text(words, length):
    out = []
    for w in [int(v) for v in words[:int(length)]]:
        letters = "".join(ALPHABET[k] for k in range(A) if (w >> k) & 1)
        out.append("x" if w == ALL_LETTERS else letters if len(letters) == 1 else f"[{letters}]")
    return "".join(out)


def _letter_bit(ch, name, col):
    k = ALPHABET.find(ch)
    if k < 0:
        raise ValueError(f"forbidden pattern {name!r}, column {col}: {ch!r} is not one of the {A} letters {ALPHABET}")
    return 1 << k


def parse_one(text):
    """One pattern's text -> list of element words. ValueError names the pattern and the column (0-based) of the fault."""
    s = str(text).strip()
    if not s:
        raise ValueError("forbidden pattern '': column 0: empty pattern")
    words, i = [], 0
    while i < len(s):
        ch, start = s[i], i
        if ch == "(":
            j = s.find(")", i)
            digits = s[i + 1:j] if j > 0 else ""
            if not words or j < 0 or not digits.isdigit() or int(digits) < 1:
                raise ValueError(f"forbidden pattern {s!r}, column {i}: a repetition is '(n)', n >= 1, behind an element")
            words.extend([words[-1]] * (int(digits) - 1))
            i = j + 1
        elif ch in "[{":
            close = "]" if ch == "[" else "}"
            j = s.find(close, i)
            if j < 0:
                raise ValueError(f"forbidden pattern {s!r}, column {i}: {ch!r} is never closed")
            bits = 0
            for c_ in range(i + 1, j):
                bits |= _letter_bit(s[c_], s, c_)
            if ch == "{":
                bits = ALL_LETTERS & ~bits
            if bits == 0:
                raise ValueError(f"forbidden pattern {s!r}, column {i}: the set {s[i:j + 1]!r} holds no letter")
            words.append(bits)
            i = j + 1
        elif ch == "x":
            words.append(ALL_LETTERS)
            i += 1
        else:
            words.append(_letter_bit(ch, s, i))
            i += 1
        if len(words) > MAX_LEN:
            raise ValueError(f"forbidden pattern {s!r}, column {start}: more than {MAX_LEN} elements")
    return words


def parse(text_or_list):
    """'N{P}[ST], NG, K(4)' or a list of such strings (a name of PRESETS stands for its pattern) -> Patterns."""
    if isinstance(text_or_list, Patterns):
        return text_or_list
    items = text_or_list.split(",") if isinstance(text_or_list, str) else list(text_or_list)
    items = [PRESETS.get(str(t).strip(), str(t).strip()) for t in items]
    if not items or (len(items) == 1 and not items[0]):
        raise ValueError("forbidden patterns: no pattern given")
    if len(items) > MAX_PATTERNS:
        raise ValueError(f"forbidden patterns: {len(items)} patterns, at most {MAX_PATTERNS}")
    elements = np.zeros((len(items), MAX_LEN), np.uint32)
    lengths = np.zeros(len(items), np.int32)
    for m, t in enumerate(items):
        words = parse_one(t)
        elements[m, :len(words)] = words
        lengths[m] = len(words)
    return Patterns(elements, lengths, items)


def check_patterns(patterns, L):
    """The argument checks of ppde_chains_set_forbidden_patterns that need no device: ValueError, or the Patterns."""
    pt = parse(patterns)
    if not 1 <= len(pt) <= MAX_PATTERNS:
        raise ValueError(f"forbidden patterns: the number of patterns must be in 1..{MAX_PATTERNS}")
    for m in range(len(pt)):
        n = int(pt.lengths[m])
        if not 1 <= n <= MAX_LEN:
            raise ValueError(f"forbidden pattern {m} ({pt.text[m]}): length must be in 1..{MAX_LEN}")
        if n > int(L):
            raise ValueError(f"forbidden pattern {m} ({pt.text[m]}): length {n} exceeds the sequence length {int(L)}")
        for j in range(n):
            w = int(pt.elements[m, j])
            if w == 0 or w >> A:
                raise ValueError(f"forbidden pattern {m} ({pt.text[m]}), element {j}: an empty set or a bit >= {A}")
    return pt


def matches(idx, patterns):
    """bool [n, M, L]: row i matches pattern m at start p (False where p + len_m > L)."""
    pt = parse(patterns)
    x = np.asarray(idx).astype(np.int64)
    x = x.reshape(-1, x.shape[-1])
    n, L = x.shape
    out = np.zeros((n, len(pt), L), bool)
    for m in range(len(pt)):
        ln = int(pt.lengths[m])
        if ln > L:
            continue
        hit = np.ones((n, L - ln + 1), bool)
        for j in range(ln):
            hit &= ((int(pt.elements[m, j]) >> x[:, j:L - ln + 1 + j]) & 1).astype(bool)
        out[:, m, :L - ln + 1] = hit
    return out


def active_mask(patterns, L, wt=None, allow_native=True):
    """bool [M, L]: pattern m is checked at start p."""
    pt = parse(patterns)
    act = np.zeros((len(pt), int(L)), bool)
    for m in range(len(pt)):
        act[m, :max(int(L) - int(pt.lengths[m]) + 1, 0)] = True
    if wt is not None and allow_native:
        act &= ~matches(np.asarray(wt).reshape(1, -1), pt)[0]
    return act


def active_words(patterns, L, wt=None, allow_native=True):
    """uint32 [L]: bit m of word p = pattern m is checked at start p (what ppde_chains_forbidden_shape returns)."""
    act = active_mask(patterns, L, wt, allow_native)
    return (act.astype(np.uint64) << np.arange(act.shape[0], dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint32)


def find(idx, patterns, wt=None, allow_native=True):
    """(first_pattern int32 [n], first_pos int32 [n]): the lowest active pattern each row matches and its lowest start; -1, -1 for a
    free row. wt None: nothing is exempt."""
    pt = parse(patterns)
    x = np.asarray(idx)
    x = x.reshape(-1, x.shape[-1])
    hit = matches(x, pt) & active_mask(pt, x.shape[1], wt, allow_native)[None]
    any_m = hit.any(axis=2)
    fp = np.where(any_m.any(axis=1), any_m.argmax(axis=1), -1).astype(np.int32)
    pos = hit[np.arange(x.shape[0]), np.maximum(fp, 0)].argmax(axis=1)
    return fp, np.where(fp >= 0, pos, -1).astype(np.int32)


def is_free(idx, patterns, wt=None, allow_native=True):
    return find(idx, patterns, wt, allow_native)[0] < 0


def summarise(vetoes, iterations, text=None):
    """vetoes int64 [n, M] after `iterations` iterations -> dict(share = proposals vetoed / proposals, per_pattern [M], text)."""
    v = np.asarray(vetoes, dtype=np.int64)
    total = max(int(v.shape[0]) * int(iterations), 1)
    per = v.sum(axis=0) / total
    return dict(share=float(per.sum()), per_pattern=per, text=list(text) if text is not None else [str(m) for m in range(v.shape[1])])


def log_line(summary):
    """'# forbidden patterns: vetoed 0.083 of the proposals so far (N{P}[ST]: 0.051, NG: 0.032)'"""
    parts = ", ".join(f"{t}: {s:.3f}" for t, s in zip(summary["text"], summary["per_pattern"]))
    return f"# forbidden patterns: vetoed {summary['share']:.3f} of the proposals so far ({parts})"


def config(patterns, allow_native=True):
    """(ppde_motif_config, the arrays it points to) for the C ABI."""
    from . import _hip
    pt = parse(patterns)
    cfg = _hip.MotifConfig(n_patterns=len(pt), length=pt.lengths.ctypes.data_as(C.POINTER(C.c_int32)),
                           element=pt.elements.ctypes.data_as(C.POINTER(C.c_uint32)), allow_native=int(bool(allow_native)))
    return cfg, pt


def scan(model, idx, patterns, allow_native=True):
    """`find` on the device (ppde_motif_scan) against the model's wild type: idx uint8 [n, L], a tensor on the model's device or
    anything numpy reads -> (first_pattern, first_pos) int32 numpy [n]."""
    import torch
    from . import _hip
    cfg, keep = config(patterns, allow_native)
    x = torch.as_tensor(np.asarray(idx) if not isinstance(idx, torch.Tensor) else idx).to(model.device, torch.uint8).contiguous()
    if x.dim() != 2 or x.shape[1] != model.L:
        raise ValueError(f"rows must be [n, {model.L}] residue indices, got {tuple(x.shape)}")
    fp = torch.empty(x.shape[0], dtype=torch.int32, device=model.device)
    pos = torch.empty_like(fp)
    with torch.cuda.device(model.device):
        torch.cuda.current_stream(model.device).synchronize()
        _hip.check(model.lib.ppde_motif_scan(model.handle, C.byref(cfg), _hip.ptr(x), int(x.shape[0]), _hip.ptr(fp), _hip.ptr(pos), None))
    del keep
    return fp.cpu().numpy(), pos.cpu().numpy()


def filter_free(model, idx, patterns, allow_native=True):
    """The rows of a candidate list that are free, by the device scan: (rows, kept bool [n])."""
    fp, _ = scan(model, idx, patterns, allow_native)
    keep = fp < 0
    return np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx)[keep], keep

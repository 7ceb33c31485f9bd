"""Helpers of the design-library tests (test_library_cpu.py, test_library_gpu.py): the MASKED reference, the enumerated
kernel over allowed moves, seeded libraries and the toy models the cases share.

The masked reference is the CPU oracle itself (oracle/ppde_oracle.py) with `forward_logits` and `categorical_probs` substituted
at run time, so that `pas_iteration` / `run` execute, for FORWARD calls only (ppde.py:98-110):
    z = forward_logits(...)                                 as the oracle forms it (range and cap masks as -inf)
    z[l, k] = -inf where the library forbids (l, k)         step 2
    p = clamp(softmax(z), 2^-23, 1 - 2^-23)                 step 3 (ppde/utils.py:106-111)
    p[l, k] = 0 where the library forbids (l, k)            step 4, before any sum of p
    p_hat = p / sum(p)                                      step 5
The reverse calls (categorical_probs(path_logits(...)), no masks) go through the oracle's own function unchanged."""
import contextlib
import itertools
import math

import numpy as np
import torch

import ppde_oracle as orc
from ppde_amd import library as dl
from ppde_amd import synthetic
from ppde_amd.encoding import seqs_to_idx

A = 20


@contextlib.contextmanager
def masked_oracle(allowed):
    """Inside the block, orc.pas_iteration / orc.run are the masked reference for library `allowed` (uint32 [L] / bool [L, 20])."""
    forbid = torch.as_tensor(~dl.as_bool(allowed)).reshape(1, -1)
    orig_fl, orig_cp = orc.forward_logits, orc.categorical_probs
    pending = {"forward": False}

    def forward_logits(*a, **k):
        z = orig_fl(*a, **k)
        pending["forward"] = True                              # the next categorical_probs call normalises these logits
        return torch.where(forbid, torch.tensor(-math.inf), z)

    def categorical_probs(z):
        fwd, pending["forward"] = pending["forward"], False
        if not fwd:
            return orig_cp(z)
        z = z - torch.logsumexp(z, dim=-1, keepdim=True)
        p = torch.softmax(z, dim=-1).clamp(min=orc.EPS, max=1.0 - orc.EPS)
        p = torch.where(forbid, torch.tensor(0.0), p)
        return p / p.sum(-1, keepdim=True)

    orc.forward_logits, orc.categorical_probs = forward_logits, categorical_probs
    try:
        yield
    finally:
        orc.forward_logits, orc.categorical_probs = orig_fl, orig_cp


def masked_run(allowed, *a, **k):
    with masked_oracle(allowed):
        return orc.run(*a, **k)


def exact_library_kernel(energy, wt_idx, allowed, pas_length, min_pos, max_pos, nmut_threshold=0):
    """The Markov kernel of ONE iteration under a design library as an explicit matrix, from the masked reference's own
    formulas (the library's counterpart of helpers.exact_pas_kernel, whose steering variates cannot make a zero-probability
    entry win): states = every combination of ALLOWED letters at the open residues (all other residues wild type), paths =
    every sequence of allowed moves. Every open residue must lie inside [min_pos, max_pos]; then no entry keeps a clamp floor
    that could be drawn (a forbidden entry has probability exactly 0 and an allowed one is never masked by the range), and the
    matrix has NO leak column: K float64 [S, S], rows summing to 1 up to rounding.
    Returns (K, states int64 [S, L], index dict: tuple of the open residues' letters -> row)."""
    wt = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    L = wt.numel()
    ok = dl.as_bool(allowed)
    positions = [int(p) for p in np.flatnonzero(ok.any(1))]
    assert positions and min_pos <= positions[0] and positions[-1] <= max_pos, "open residues must lie inside the range"
    thr = np.iinfo(np.int32).max if nmut_threshold == 0 else nmut_threshold
    choices = [list(np.flatnonzero(ok[p])) for p in positions]
    combos = list(itertools.product(*choices))
    index = {tuple(int(v) for v in c): i for i, c in enumerate(combos)}
    S = len(combos)
    states = wt.repeat(S, 1)
    states[:, positions] = torch.as_tensor(np.array(combos, dtype=np.int64))
    moves = np.array([p * A + k for p, ch in zip(positions, choices) for k in ch], dtype=np.int64)
    K = np.zeros((S, S))
    n_len = 2 * pas_length - 1
    wt_row = index[tuple(int(wt[p]) for p in positions)]
    with masked_oracle(allowed):
        for x in range(S):
            for U in range(1, n_len + 1):
                paths = np.array(list(itertools.product(range(len(moves)), repeat=U)), dtype=np.int64)
                flat = moves[paths]
                c = flat.shape[0]
                q = torch.full((U, c, L * A), 1e30)
                for s in range(U):
                    q[s, torch.arange(c), torch.as_tensor(flat[:, s])] = 1e-30
                start = states[x].repeat(c, 1)
                out = orc.pas_iteration(energy, start, start, wt, torch.full((c,), U, dtype=torch.int64), q, torch.full((c,), 0.5),
                                        min_pos, max_pos, thr, keep_probs=True)
                assert np.array_equal(out["flat"].numpy().T, flat), "the steering variates did not select the wanted path"
                pf = out["p_fwd"].double().numpy()
                p_path = np.prod([pf[s, np.arange(c), flat[:, s]] for s in range(U)], axis=0)
                a = np.minimum(1.0, np.exp(out["log_acc"].double().numpy()))
                end = out["proposal"].clone()
                end[(end != wt).sum(1) >= thr] = wt                                                   # accepted, then reset
                y = np.array([index[tuple(int(v) for v in row)] for row in end[:, positions].numpy()])
                stay = wt_row if int((states[x] != wt).sum()) >= thr else x
                w = p_path / n_len
                np.add.at(K[x], y, w * a)
                K[x, stay] += float((w * (1.0 - a)).sum())
    return K, states, index


def state_cells(idx, allowed, index, start_row):
    """Rows of K for a population idx [n, L] (every chain started from `start_row`'s state), and the number of chains on a
    FORBIDDEN state: a letter outside the library at an open residue, or a frozen residue that moved."""
    ok = dl.as_bool(allowed)
    idx = np.asarray(idx).astype(np.int64)
    positions = np.flatnonzero(ok.any(1))
    frozen = np.setdiff1d(np.arange(idx.shape[1]), positions)
    bad = (idx[:, frozen] != np.asarray(start_row).astype(np.int64)[frozen][None]).any(1)
    bad |= ~ok[positions[None, :], idx[:, positions]].all(1)
    cells = np.array([index.get(tuple(int(v) for v in r), -1) for r in idx[:, positions]])
    return cells, int((bad | (cells < 0)).sum())


def chi_square(counts, expected, floor=8.0):
    """tests/test_sampler_law.py's statistic: Pearson, cells with an expectation below `floor` merged into one."""
    small = expected < floor
    O = np.append(counts[~small], counts[small].sum())
    E = np.append(expected[~small], expected[small].sum())
    keep = E > 0
    O, E = O[keep], E[keep]
    return float(((O - E) ** 2 / E).sum()), len(E) - 1


def chi_square_bound(df):
    return df + 5.0 * np.sqrt(2.0 * df)


def seeded_library(wt_idx, lo, hi, seed, frozen_fraction=1.0 / 3.0):
    """A library over the window lo..hi: about `frozen_fraction` of its residues frozen (a non-contiguous choice), every
    other one with 2..20 letters, its wild-type letter among them; everything outside the window frozen."""
    wt = np.asarray(wt_idx).astype(np.int64)
    rng = np.random.default_rng(seed)
    out = np.zeros(wt.shape[0], np.uint32)
    for l in range(lo, hi + 1):
        if rng.random() < frozen_fraction:
            continue
        k = int(rng.integers(2, A + 1))
        letters = set(rng.choice(A, size=k, replace=False).tolist()) | {int(wt[l])}
        out[l] = sum(1 << int(v) for v in letters)
    assert out.any() and (out[lo:hi + 1] == 0).any()
    return out


def law_case(seed=31):
    """The law tests' model: L = 7, Potts window 0..5, residues 2 and 3 open with 7 and 5 letters (wild type included)."""
    L, Lp, i0 = 7, 6, 0
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, sigma_J=0.3, sigma_h=0.8)
    allowed = np.zeros(L, np.uint32)
    for site, count in ((2, 7), (3, 5)):
        others = [k for k in rng.permutation(A).tolist() if k != int(wt[site])][:count - 1]
        allowed[site] = sum(1 << k for k in others) | (1 << int(wt[site]))
    assert [bin(int(w)).count("1") for w in allowed[[2, 3]]] == [7, 5]
    return dict(L=L, Lp=Lp, i0=i0, wt=wt, J=J, h=h, allowed=allowed)


def toy24(lamda=5.0):
    """TOY24 with the synthetic Potts + CNN experts of the other parity tests."""
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    wt = seqs_to_idx([seq])[0]
    J, h = synthetic.make_potts(Lp, seed=7)
    cnn = [synthetic.make_cnn_state(len(seq), s) for s in range(3)]
    return dict(L=len(seq), Lp=Lp, i0=i0, wt=wt, J=J, h=h, cnn=cnn, lamda=lamda)


def potts_case(L, i0, Lp, seed):
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, sigma_J=0.1, sigma_h=0.5)
    return dict(L=L, Lp=Lp, i0=i0, wt=wt, J=J, h=h, cnn=None, lamda=0.0)


def oracle_energy_of(case):
    P = orc.PottsOracle(case["J"], case["h"], case["i0"], torch.as_tensor(case["wt"].astype(np.int64)))
    C = orc.CnnOracle(case["cnn"]) if case.get("cnn") is not None else None
    return orc.EnergyOracle(P, C, case.get("lamda", 0.0))


def hip_model_of(case):
    from ppde_amd.energy import HipModel
    m = HipModel(case["wt"], "cuda:0")
    m.set_potts(case["J"], case["h"], case["i0"])
    if case.get("cnn") is not None:
        m.set_cnn(case["cnn"])
    m.set_lamda(case.get("lamda", 0.0))
    return m

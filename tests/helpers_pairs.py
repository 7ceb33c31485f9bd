"""The reference of the pair counts (ppde_chains_set_pair_counts): one function, an integer bincount, plus the seeded start
populations and site lists tests/test_pairs_gpu.py runs from (tests/test_pairs_cpu.py shows that they can see a transposed kernel)."""
import numpy as np

A = 20
GEOMETRIES = ((8, 1, 6), (70, 62, 6), (104, 98, 6), (237, 200, 6))        # (L, i0, Lp): tests/test_recorder_gpu.py's layout edges
POPULATIONS = (1, 63, 64, 65, 130, 257)
SITE_COUNTS = (1, 3, 4, 5, 8, 9, 17)                                       # ragged tiles for a tile side of 4 or 8


def pair_counts_of(idx, sites):
    """idx [rows, slots, L] letters, sites [S] residues -> uint64 [S, 20, S, 20]: counts[i, a, j, b] = number of (row, slot) pairs
    with letter a at residue sites[i] and letter b at residue sites[j]."""
    idx = np.asarray(idx)
    sites = np.asarray(sites, dtype=np.int64).reshape(-1)
    x = idx.reshape(-1, idx.shape[-1])[:, sites].astype(np.int64)          # [samples, S]
    S = sites.size
    W = S * A
    key = np.arange(S, dtype=np.int64)[None, :] * A + x                    # row of the one-hot matrix each (sample, site) sets
    out = np.zeros(W * W, np.int64)
    step = max(1, (1 << 22) // (S * S))                                    # samples per pass: about 4M bin indices at a time
    for lo in range(0, key.shape[0], step):
        k = key[lo:lo + step]
        out += np.bincount((k[:, :, None] * W + k[:, None, :]).ravel(), minlength=W * W)
    return out.astype(np.uint64).reshape(S, A, S, A)


def random_population(n, L, seed):
    """Uniformly random letters: a run from the wild type leaves almost every bin empty and cannot see an index error."""
    return np.random.default_rng(seed).integers(0, A, size=(n, L)).astype(np.uint8)


def scattered_sites(L, S, seed):
    """S strictly increasing residues of 0..L-1 that include the first and the last one (S = 1: the last)."""
    if S == 1:
        return np.array([L - 1], np.int32)
    S = min(S, L)
    inner = np.random.default_rng(seed).choice(np.arange(1, L - 1), size=S - 2, replace=False)
    return np.sort(np.concatenate([[0, L - 1], inner])).astype(np.int32)


def site_lists(L, seed=0):
    """None (every residue) and the scattered lists of the GPU test for a sequence of L."""
    return [None] + [scattered_sites(L, S, seed + S) for S in SITE_COUNTS if S <= L]


def start_population(L, n):
    """The seeded random start of the GPU test's case (L, n)."""
    return random_population(n, L, 9000 + 7 * L + n)

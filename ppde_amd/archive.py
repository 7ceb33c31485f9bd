"""Host side of the per-chain archives (include/ppde_hip.h, ppde_chains_set_archive): the population's distinct candidates.

The device keeps K entries per chain and never looks across chains; n K rows are cheap to merge here.
"""
import numpy as np


def merge(idx, energy, fitness, step, count, chain_offset=0):
    """Distinct states over the archives of n chains: idx uint8 [n, K, L], energy / fitness [n, K], step [n, K], count [n] as
    `Chains.archive()` returns them; chain_offset is the global index of chain 0. One row per distinct state: the entry with the
    highest energy, then the lowest global chain, then the lowest step; n_chains = number of chains whose archive holds the
    state. Sorted by (energy descending, chain ascending, step ascending). Returns a dict of idx uint8 [M, L], energy / fitness
    fp32 [M], chain int64 [M], step int32 [M], n_chains int32 [M]."""
    idx = np.asarray(idx, np.uint8)
    n, K, L = idx.shape
    energy = np.asarray(energy, np.float32).reshape(n, K)
    fitness = np.asarray(fitness, np.float32).reshape(n, K)
    step = np.asarray(step, np.int32).reshape(n, K)
    count = np.asarray(count).reshape(n)
    if (count < 0).any() or (count > K).any():
        raise ValueError(f"merge: count must lie in 0..{K}")
    live = np.arange(K)[None, :] < count[:, None]
    b, j = np.nonzero(live)
    rows, e, f, s = idx[b, j], energy[b, j], fitness[b, j], step[b, j]
    chain = b.astype(np.int64) + int(chain_offset)
    order = np.lexsort((s, chain, -e.astype(np.float64)))                   # energy descending, chain, step ascending
    rows, e, f, s, chain = rows[order], e[order], f[order], s[order], chain[order]
    first, n_chains = {}, []
    keep = []
    for i in range(rows.shape[0]):                                           # (the first occurrence in this order is the kept entry)
        key = rows[i].tobytes()
        at = first.get(key)
        if at is None:
            first[key] = len(keep)
            keep.append(i)
            n_chains.append({int(chain[i])})
        else:
            n_chains[at].add(int(chain[i]))
    keep = np.asarray(keep, np.int64)
    return dict(idx=rows[keep].reshape(-1, L), energy=e[keep], fitness=f[keep], chain=chain[keep], step=s[keep],
                n_chains=np.asarray([len(c) for c in n_chains], np.int32))

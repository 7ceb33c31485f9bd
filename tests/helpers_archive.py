"""The reference of the per-chain archive (ppde_chains_set_archive, include/ppde_hip.h): the online rule restated on a list of
`peek()` dicts, the offline answer it must agree with when energy is a function of the state, and counters of what the rule did
on a given run (so a test can assert that the branch it means to check was taken).

A peek is a dict of idx uint8 [n, L], energy fp32 [n], fitness fp32 [n], dist int [n]; peeks[t] is the population after t
completed iterations. Energies are compared as fp32, like the device."""
import numpy as np

KMAX = 32


def _walk(peeks, K):
    n, L = np.asarray(peeks[0]["idx"]).shape
    entries = [[] for _ in range(n)]                    # per chain: [bytes, energy, fitness, step]
    ev = dict(insertions=0, evictions=0, equal_refusals=0, lower_refusals=0, duplicates=0, changed_duplicates=0, wt_skips=0,
              nonfinite_skips=0)
    for t, pk in enumerate(peeks):
        idx, e, f, dist = (np.asarray(pk[k]) for k in ("idx", "energy", "fitness", "dist"))
        e, f = e.astype(np.float32), f.astype(np.float32)
        prev = np.asarray(peeks[t - 1]["idx"]) if t else None
        for b in range(n):
            if int(dist[b]) == 0:
                ev["wt_skips"] += 1
                continue
            if not np.isfinite(e[b]):
                ev["nonfinite_skips"] += 1
                continue
            key, ent = idx[b].tobytes(), entries[b]
            if any(x[0] == key for x in ent):
                ev["duplicates"] += 1
                if prev is not None and (prev[b] != idx[b]).any():
                    ev["changed_duplicates"] += 1
                continue
            new = [key, e[b], f[b], t]
            if len(ent) < K:
                ent.append(new)
                ev["insertions"] += 1
                continue
            m = min(range(K), key=lambda j: (ent[j][1], -ent[j][3]))         # lowest energy, the latest step among equals
            if e[b] > ent[m][1]:
                ent[m] = new
                ev["evictions"] += 1
            elif e[b] == ent[m][1]:
                ev["equal_refusals"] += 1
            else:
                ev["lower_refusals"] += 1
    ev["short_chains"] = sum(1 for ent in entries if len(ent) < K)
    return entries, ev, n, L


def archive_of(peeks, K):
    """The online rule on a list of peeks, returned as ppde_chains_archive_read returns it: idx uint8 [n, K, L], energy /
    fitness fp32 [n, K], step int32 [n, K], count int32 [n]; entries by (energy descending, step ascending), the slots beyond
    count filled with 255, -inf, 0, -1."""
    entries, _, n, L = _walk(peeks, K)
    out = dict(idx=np.full((n, K, L), 255, np.uint8), energy=np.full((n, K), -np.inf, np.float32),
               fitness=np.zeros((n, K), np.float32), step=np.full((n, K), -1, np.int32), count=np.zeros(n, np.int32))
    for b, ent in enumerate(entries):
        ent = sorted(ent, key=lambda x: (-float(x[1]), x[3]))
        out["count"][b] = len(ent)
        for j, (key, e, f, t) in enumerate(ent):
            out["idx"][b, j] = np.frombuffer(key, np.uint8)
            out["energy"][b, j], out["fitness"][b, j], out["step"][b, j] = e, f, t
    return out


def events(peeks, K):
    """What the rule did on these peeks: insertions, evictions, equal_refusals (a full archive, a new state, e == the minimum),
    lower_refusals, duplicates, changed_duplicates (a duplicate at an iteration where the chain's state differs from the
    iteration before: a real revisit, not a rejected move), wt_skips, nonfinite_skips, short_chains (count < K at the end)."""
    return _walk(peeks, K)[1]


def top_distinct(states, e, dist, K):
    """Offline: the K highest-energy distinct non-wild-type states of ONE chain's history (states [T+1, L], e [T+1], dist [T+1]),
    as a set of byte strings. Meaningful when energy is a function of the state and distinct states have distinct energies."""
    best = {}
    for s, v, d in zip(np.asarray(states, np.uint8), np.asarray(e, np.float32), np.asarray(dist)):
        if int(d) == 0 or not np.isfinite(v):
            continue
        best.setdefault(s.tobytes(), v)
    return set(sorted(best, key=lambda k: -float(best[k]))[:K])


def peeks_of(states, e_hist, f_hist, wt):
    """Peeks of a CPU reference run: states [T+1, n, L] (post-reset), histories [T+1, n], the wild type [L]."""
    states, wt = np.asarray(states).astype(np.uint8), np.asarray(wt).astype(np.uint8)
    return [dict(idx=states[t], energy=np.asarray(e_hist[t], np.float32), fitness=np.asarray(f_hist[t], np.float32),
                 dist=(states[t] != wt[None]).sum(1).astype(np.int32)) for t in range(states.shape[0])]


def hand_peeks(rows, wt):
    """Peeks of ONE chain from a list of (letters, energy): fitness = -energy, dist from the wild type `wt`."""
    wt = np.asarray(wt, np.uint8)
    out = []
    for s, e in rows:
        s = np.asarray(s, np.uint8)
        with np.errstate(invalid="ignore"):
            out.append(dict(idx=s[None], energy=np.asarray([e], np.float32), fitness=-np.asarray([e], np.float32),
                            dist=np.asarray([(s != wt).sum()], np.int32)))
    return out


# ------------------------------------------------------------------------------------------------ the layout-edge geometries
EDGE_LENGTHS = (8, 70, 104, 237, 252, 253, 307)
EDGE_POPULATIONS = (1, 3, 4, 5, 65)
EDGE_K, EDGE_T = 4, 60


def edge_case(L, seed=None):
    """Potts-only geometry of length L for the layout-edge tests: the Potts window starts after residue 1 and ends before L - 2, so
    states that differ only at residues 0, 1, L - 2, L - 1 share an energy. The library opens those four and two residues astride
    a dword boundary of the state row (the boundary between the two dwords a lane holds, byte 256, where the row reaches it; the
    middle of the row otherwise), with 2 to 3 letters each. Returns (case, library uint32 [L], open residues)."""
    import helpers_library as hl
    i0, Lp = 2, L - 4
    c = hl.potts_case(L, i0, Lp, 900 + L if seed is None else seed)
    sh = (4 - (i0 & 3)) & 3                              # byte of residue 0 in a state row (set_geom in ppde_api.hip)
    first = 255 - sh if 255 - sh + 1 <= L - 3 else max(l for l in range(1, L // 2 + 2) if (sh + l) % 4 == 3)
    assert (sh + first) % 4 == 3 and first + 1 < L
    sites = sorted({0, 1, L - 2, L - 1, first, first + 1})
    rng = np.random.default_rng(1000 + L)
    lib = np.zeros(L, np.uint32)
    for l in sites:
        others = [k for k in rng.permutation(20).tolist() if k != int(c["wt"][l])][:int(rng.integers(1, 3))]
        lib[l] = sum(1 << k for k in others) | (1 << int(c["wt"][l]))
    return c, lib, sites

"""Host side of recombination (include/ppde_hip.h, ppde_chains_set_recombination): what the recorded events say, in plain numpy.

The raw arrays, as `Chains.recombination_state()` holds them, [events, n] each: partner (index of the other chain of the pair), lo, hi
(the cut, as indices into the open list), differ (segment residues at which the two parents differ), child_dist, outcome
(0 rejected by the test against u, 1 accepted, 2 a child at the mutation cap, 3 a non-finite child energy, 4 a child that matches
a forbidden pattern: only with ppde_chains_set_forbidden_patterns), log_ratio, pre_energy, child_energy."""
import numpy as np

REJECTED, ACCEPTED, CAPPED, NOT_FINITE, FORBIDDEN = 0, 1, 2, 3, 4


def _pairs(records):
    """One row per pair (the slot that is lower than its partner): dict of flat arrays lo, hi, differ, outcome."""
    partner = np.asarray(records["partner"])
    first = np.arange(partner.shape[-1])[None] < partner
    return {k: np.asarray(records[k])[first] for k in ("lo", "hi", "differ", "outcome")}


def _rate(acc, sel):
    return float(acc[sel].mean()) if sel.any() else float("nan")


def summarise(records):
    """Acceptance of the recorded pairs. Pairs whose parents agree on the whole segment (differ = 0) are always accepted and
    change nothing: they are counted apart, and every acceptance rate is over the pairs with differ > 0.
    Returns pairs, identical_share, acceptance, capped_share, not_finite_share, forbidden_share (shares of all pairs), by_length {hi - lo + 1:
    (pairs, acceptance)} and by_differ {differ: (pairs, acceptance)}."""
    p = _pairs(records)
    n = int(p["outcome"].size)
    if n == 0:
        return dict(pairs=0, identical_share=float("nan"), acceptance=float("nan"), capped_share=float("nan"),
                    not_finite_share=float("nan"), forbidden_share=float("nan"), by_length={}, by_differ={})
    acc = p["outcome"] == ACCEPTED
    real = p["differ"] > 0
    length = p["hi"] - p["lo"] + 1
    by_length = {int(v): (int((real & (length == v)).sum()), _rate(acc, real & (length == v))) for v in np.unique(length[real])}
    by_differ = {int(v): (int((p["differ"] == v).sum()), _rate(acc, p["differ"] == v)) for v in np.unique(p["differ"][real])}
    return dict(pairs=n, identical_share=float((~real).mean()), acceptance=_rate(acc, real),
                capped_share=float((p["outcome"] == CAPPED).mean()), not_finite_share=float((p["outcome"] == NOT_FINITE).mean()),
                forbidden_share=float((p["outcome"] == FORBIDDEN).mean()), by_length=by_length, by_differ=by_differ)


def lineage(records, open_sites, n, L):
    """int32 [n, L]: for every slot and residue at the end of the run, the index of the INITIAL chain that position descends from
    through the accepted exchanges (mutations inside a chain keep the position's founder): the mosaic a candidate's parentage is
    read from. Partner indices and slots share one numbering (local to an object, global after a gather)."""
    open_sites = np.asarray(open_sites, dtype=np.int64)
    partner, lo, hi, outcome = (np.asarray(records[k]) for k in ("partner", "lo", "hi", "outcome"))
    who = np.tile(np.arange(n, dtype=np.int32)[:, None], (1, L))
    for ev in range(partner.shape[0]):
        for a in np.flatnonzero((outcome[ev] == ACCEPTED) & (np.arange(n) < partner[ev])):
            b = int(partner[ev, a])
            seg = open_sites[int(lo[ev, a]):int(hi[ev, a]) + 1]
            who[a, seg], who[b, seg] = who[b, seg].copy(), who[a, seg].copy()
    return who

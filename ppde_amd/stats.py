"""Host side of the move statistics (include/ppde_hip.h, ppde_chains_set_stats): what the counters say, in plain numpy.

The raw arrays, int64, as `Chains.stats()` returns them: iters, accepts, moved, jump_sum, dist_sum, wt_returns [n, R'],
len_attempts, len_accepts [R', M], site_changes [R', L] or None; R' = max(rungs, 1), M = 2 pas_length - 1."""
import numpy as np

PER_CHAIN = ("iters", "accepts", "moved", "jump_sum", "dist_sum", "wt_returns")
PER_LENGTH = ("len_attempts", "len_accepts")
KEYS = PER_CHAIN + PER_LENGTH + ("site_changes",)


def _ratio(a, b):
    """a / b as float64, nan where b == 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def summarise(raw, betas=None):
    """Rates of a run from its raw counters (a dict with KEYS; site_changes may be None). Ratios with an empty denominator are nan.
        acceptance              accepts / iters over everything
        acceptance_by_rung      [R']      acceptance_by_chain [n]
        acceptance_by_length    [R', M]   len_accepts / len_attempts: row r, column U - 1
        mean_jump               [R']      residues changed per ACCEPTED iteration (jump_sum / accepts)
        moved_fraction          [R']      iterations that changed the state / iterations
        mean_dist               [R']      mean mutation count after an iteration
        wt_returns_per_1000     [R']      returns to the wild type per 1000 iterations
        site_mobility           [R', L]   site_changes / iterations on the rung (None without per-site counts)
        betas                   [R'] or None, as given"""
    r = {k: np.asarray(raw[k], np.int64) for k in PER_CHAIN + PER_LENGTH}
    it_r, acc_r = r["iters"].sum(0), r["accepts"].sum(0)
    out = dict(
        acceptance=float(_ratio(r["accepts"].sum(), r["iters"].sum())),
        acceptance_by_rung=_ratio(acc_r, it_r),
        acceptance_by_chain=_ratio(r["accepts"].sum(1), r["iters"].sum(1)),
        acceptance_by_length=_ratio(r["len_accepts"], r["len_attempts"]),
        mean_jump=_ratio(r["jump_sum"].sum(0), acc_r),
        moved_fraction=_ratio(r["moved"].sum(0), it_r),
        mean_dist=_ratio(r["dist_sum"].sum(0), it_r),
        wt_returns_per_1000=1000.0 * _ratio(r["wt_returns"].sum(0), it_r),
        site_mobility=None if raw.get("site_changes") is None else _ratio(np.asarray(raw["site_changes"], np.int64), it_r[:, None]),
        betas=None if betas is None else np.asarray(betas, np.float32).copy())
    return out


def log_line(raw, max_lengths=6):
    """The periodic log's line: overall acceptance so far and acceptance by path length over all rungs."""
    att, acc = np.asarray(raw["len_attempts"]).sum(0), np.asarray(raw["len_accepts"]).sum(0)
    by_len = ", ".join(f"{u + 1}: {acc[u] / att[u]:.2f}" for u in range(min(att.size, max_lengths)) if att[u])
    total = att.sum()
    return f"   # acceptance so far = {(acc.sum() / total if total else float('nan')):.3f} (path length {by_len})"

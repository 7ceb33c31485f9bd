"""The reference of the move statistics (ppde_chains_set_stats, include/ppde_hip.h): the rule restated on the peeks of a run, and
counters of which branches a run took (so a test can assert that the branch it means to check was taken).

peeks[t] is the population after t completed iterations as `Chains.peek()` returns it (idx uint8 [n, L], dist int [n]); accepted
and U are [T, n] (the trace's accepted and U); rung_history is [T + 1, n] (row it: the rungs the chains ran iteration it on)."""
import numpy as np

PER_CHAIN = ("iters", "accepts", "moved", "jump_sum", "dist_sum", "wt_returns")
KEYS = PER_CHAIN + ("len_attempts", "len_accepts", "site_changes")


def stats_of(peeks, accepted, U, rung_history=None, n_rungs=0, mu_max=3):
    """The nine counters of include/ppde_hip.h after len(peeks) - 1 iterations, int64."""
    n, L = np.asarray(peeks[0]["idx"]).shape
    R, b = max(int(n_rungs), 1), np.arange(n)
    out = {k: np.zeros((n, R), np.int64) for k in PER_CHAIN}
    out.update(len_attempts=np.zeros((R, mu_max), np.int64), len_accepts=np.zeros((R, mu_max), np.int64),
               site_changes=np.zeros((R, L), np.int64))
    for it in range(len(peeks) - 1):
        changed = np.asarray(peeks[it]["idx"]) != np.asarray(peeks[it + 1]["idx"])
        h, A, u = changed.sum(1), np.asarray(accepted[it]).astype(np.int64), np.asarray(U[it]).astype(np.int64)
        d0, d1 = np.asarray(peeks[it]["dist"]).astype(np.int64), np.asarray(peeks[it + 1]["dist"]).astype(np.int64)
        r = np.asarray(rung_history[it]).astype(np.int64) if n_rungs else np.zeros(n, np.int64)
        for k, v in (("iters", 1), ("accepts", A), ("moved", h > 0), ("jump_sum", h), ("dist_sum", d1), ("wt_returns", (d0 > 0) & (d1 == 0))):
            np.add.at(out[k], (b, r), v)
        np.add.at(out["len_attempts"], (r, u - 1), 1)
        np.add.at(out["len_accepts"], (r, u - 1), A)
        bi, li = np.nonzero(changed)
        np.add.at(out["site_changes"], (r[bi], li), 1)
    return out


def events(peeks, accepted, U, rung_history=None, n_rungs=0, mu_max=3):
    """Which branches a run took: acc_by_len / rej_by_len [mu_max] (accepted / rejected iterations at each path length),
    wt_returns, short_jumps (accepted, 0 < h < U), still_accepts (accepted, h == 0), moved_without_accept (h > 0, not accepted),
    rung_moves ((chain, iteration) whose rung after the swap differs from the one it iterated on), changed_sites (residues that
    changed at least once)."""
    T = len(peeks) - 1
    idx = np.stack([np.asarray(p["idx"]) for p in peeks])
    dist = np.stack([np.asarray(p["dist"]) for p in peeks]).astype(np.int64)
    A, u = np.asarray(accepted[:T]).astype(bool), np.asarray(U[:T]).astype(np.int64)
    changed = idx[1:] != idx[:-1]
    h = changed.sum(2)
    return dict(acc_by_len=np.array([int((A & (u == k)).sum()) for k in range(1, mu_max + 1)]),
                rej_by_len=np.array([int((~A & (u == k)).sum()) for k in range(1, mu_max + 1)]),
                wt_returns=int(((dist[:-1] > 0) & (dist[1:] == 0)).sum()),
                short_jumps=int((A & (h > 0) & (h < u)).sum()), still_accepts=int((A & (h == 0)).sum()),
                moved_without_accept=int((~A & (h > 0)).sum()),
                rung_moves=int((np.asarray(rung_history[1:T + 1]) != np.asarray(rung_history[:T])).sum()) if n_rungs else 0,
                changed_sites=np.flatnonzero(changed.any((0, 1))))


def assert_identities(st, steps_done, paper=False):
    """The identities of include/ppde_hip.h on a dict of the nine counters (site_changes may be None)."""
    assert (st["iters"].sum(1) == steps_done).all()
    assert np.array_equal(st["iters"].sum(0), st["len_attempts"].sum(1)) and np.array_equal(st["accepts"].sum(0), st["len_accepts"].sum(1))
    if st["site_changes"] is not None:
        assert np.array_equal(st["site_changes"].sum(1), st["jump_sum"].sum(0))
    assert (st["len_accepts"] <= st["len_attempts"]).all() and (st["moved"] <= st["jump_sum"]).all()
    assert all((st[k] >= 0).all() for k in KEYS if st[k] is not None)
    if not paper:
        assert (st["moved"] <= st["accepts"]).all()

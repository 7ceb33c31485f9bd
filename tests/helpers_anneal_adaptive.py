"""The reference of adaptive population annealing (ppde_chains_set_annealing_adaptive; tests/test_anneal_adaptive_cpu.py,
tests/test_anneal_adaptive_gpu.py): the step of one deme, restated from include/ppde_hip.h in fp64 numpy, and the whole run built
on helpers_anneal.annealed_run and helpers_anneal.plan.

    b0 = (double)beta_cur; e_i the fp32 post-accept energies, F the finite ones, E_max their maximum, x_i = e_i - E_max;
    F == 0 or dmax = (double)beta_end - b0 <= 0: beta stays;
    ESS(d) = (sum exp(d x_i))^2 / sum exp(2 d x_i), target = (double)rho F;
    ESS(dmax) >= target: d = dmax; otherwise 48 bisections of [0, dmax] (ESS(mid) >= target ? lo = mid : hi = mid) and
    d = max(lo, (double)min_step); beta_next = beta_end if d >= dmax or (float)(b0 + d) >= beta_end, else (float)(b0 + d);
    the event then runs helpers_anneal.plan with dbeta = (double)beta_next - b0.

Planted faults, and the comparison of tests/test_anneal_adaptive_gpu.py that rejects each (shown on the CPU by
test_anneal_adaptive_cpu.test_every_planted_fault_is_rejected_by_the_gpu_comparison):
    target_D   target rho D where F < D            the step test: beta_next more than one fp32 ulp from the rule (cases with F < D;
                                                   on the device that branch is covered by the rule and by reading the kernel)
    no_shift   energies not shifted by E_max       the step test: exp overflows where the energies are large (ESS is nan and the
                                                   bisection backs off), beta_next is off
    hi         the bisection returns hi            the step test at one ulp where the bracket is wider than an ulp -- it is not after
                                                   48 halvings, so this fault is planted with 8 halvings ('hi8'), as a stand-in for
                                                   any early exit from the loop; with all 48 the two ends round to the same fp32
    no_floor   min_step ignored                    the step test on the events the floor decides
    delta_w    resampling weights from d, not from the fp32-rounded beta_next - beta_cur: beta_next is right, so the step
               comparison passes; log_mean_w and ess differ from helpers_anneal.plan on the recorded beta pair beyond 1e-12
               (the plan's criteria see it), and the fixed-schedule replay, which compares the whole run bit for bit, is the
               test whose purpose it is."""
import numpy as np

import helpers_anneal as ha

FAULTS = ("target_D", "no_shift", "hi8", "no_floor", "delta_w")
ORDERS = ("pairwise", "forward", "backward")


def _sum(v, order):
    if order == "pairwise":
        return np.float64(np.sum(v))
    if order == "forward":
        return np.float64(np.cumsum(v)[-1])
    return np.float64(np.cumsum(v[::-1])[-1])                                # (numpy scalars: an overflow is inf, not an exception)


def ess_of(x, d, order="pairwise"):
    """ESS(d) of the shifted finite energies x (fp64)."""
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(d * x)
        return float(_sum(w, order) ** 2 / _sum(w * w, order))


def step(e, beta_cur, beta_end, rho, min_step, fault=None, order="pairwise"):
    """The step of one deme. e fp32 [D]; the other arguments as fp32. Returns dict(beta_next fp32, db fp64 = the plan's dbeta,
    delta, by in ('empty', 'arrived', 'jump', 'bisect', 'floor'), F, target, x, dmax)."""
    e32 = np.asarray(e, np.float32)
    b_cur, b_end = np.float32(beta_cur), np.float32(beta_end)
    b0 = float(b_cur)
    fin = np.isfinite(e32)
    F = int(fin.sum())
    out = dict(beta_next=b_cur, db=0.0, delta=0.0, by="empty", F=F, target=float(np.float32(rho)) * F, x=None, dmax=float(b_end) - b0)
    if F == 0:
        return out
    dmax = float(b_end) - b0
    if dmax <= 0.0:
        out["by"] = "arrived"
        return out
    ed = e32[fin].astype(np.float64)
    x = ed if fault == "no_shift" else ed - ed.max()
    target = float(np.float32(rho)) * (e32.size if fault == "target_D" else F)
    by = "jump"
    d = dmax
    if not ess_of(x, dmax, order) >= target:
        lo, hi = 0.0, dmax
        for _ in range(8 if fault == "hi8" else 48):
            mid = 0.5 * (lo + hi)
            if ess_of(x, mid, order) >= target:
                lo = mid
            else:
                hi = mid
        d = hi if fault == "hi8" else lo
        by = "bisect"
        if fault != "no_floor" and float(np.float32(min_step)) >= d:
            d, by = float(np.float32(min_step)), "floor"
    b_try = np.float32(b0 + d)
    if d >= dmax or b_try >= b_end:
        b_next = b_end
        by = by if by == "jump" else by + "+arrival"
    else:
        b_next = b_try
    out.update(beta_next=b_next, db=d if fault == "delta_w" else float(b_next) - b0, delta=d, by=by, target=target, x=x)
    return out


def ulp32(b):
    return float(np.spacing(np.float32(b)))


def adaptive_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length, nmut_threshold, beta_start, beta_end, rho,
                 min_step, every, deme, max_stages=4096, seed=0, chain_offset=0, allowed=None, fault=None, trace=False, keep_probs=False, forbidden=None,
                 motif_fault=None):
    """The adaptive run of ONE deme (idx0 [D, L]; `noise` as helpers_anneal.annealed_run takes it) by the rule itself: the schedule
    is grown one event at a time -- annealed_run on the path so far (padded with an equal beta, whose event is the identity)
    shows the energies event s sees, `step` turns them into beta_after[s] -- and the run on the finished path is returned with
    beta_path fp32 [events + 1]. `fault`: one of FAULTS ('delta_w' resamples event s by helpers_anneal.plan's weights at d
    instead of at the rounded pair; the others change beta_next). `trace`, `keep_probs`: as annealed_run takes them, for the
    returned run. `forbidden`, `motif_fault`: handed to every annealed_run (the prefixes run under the constraint too)."""
    D = int(deme)
    assert idx0.shape[0] == D
    cap = min(int(max_stages), num_steps // every)
    path = [np.float32(beta_start)]
    db_over = {}

    def run(sched, T, **kw):
        if forbidden is not None:
            kw.update(forbidden=forbidden, motif_fault=motif_fault)
        if fault != "delta_w":
            return ha.annealed_run(energy, idx0, wt_idx, noise, T, min_pos, max_pos, pas_length, nmut_threshold, sched, every, D, seed=seed,
                                   chain_offset=chain_offset, allowed=allowed, **kw)
        return _run_with_db(energy, idx0, wt_idx, noise, T, min_pos, max_pos, pas_length, nmut_threshold, sched, every, D, seed,
                            chain_offset, allowed, db_over, **kw)

    for s in range(cap):
        r = run(np.array(path + [path[-1]], np.float32), (s + 1) * every)
        st = step(r["pre_energy"][s], path[-1], beta_end, rho, min_step, fault=fault)
        db_over[s] = st["db"]
        path.append(st["beta_next"])
    res = run(np.array(path, np.float32), num_steps, trace=trace, keep_probs=keep_probs)
    res["beta_path"] = np.array(path, np.float32)
    return res


def _run_with_db(energy, idx0, wt_idx, noise, T, min_pos, max_pos, pas_length, nmut_threshold, sched, every, D, seed, chain_offset,
                 allowed, db_over, **kw):
    """annealed_run whose plan of event s takes dbeta = db_over[s] where given (the 'delta_w' fault): helpers_anneal.plan is
    wrapped for the duration of the call."""
    real, calls = ha.plan, [0]

    def plan(e, dbeta, u, fault=None):
        s = calls[0]
        calls[0] += 1
        return real(e, db_over.get(s, dbeta), u, fault=fault)

    ha.plan = plan
    try:
        return ha.annealed_run(energy, idx0, wt_idx, noise, T, min_pos, max_pos, pas_length, nmut_threshold, sched, every, D, seed=seed,
                               chain_offset=chain_offset, allowed=allowed, **kw)
    finally:
        ha.plan = real


def check_event(pre_energy, beta_before, beta_after, beta_end, rho, min_step, u, parent, log_mean_w, ess):
    """The comparison tests/test_anneal_adaptive_gpu.py makes for one event of one deme, on recorded arrays: beta_after within
    one fp32 ulp of the numpy step on pre_energy; parent equal to helpers_anneal.plan's on the recorded beta pair wherever every
    offspring is decided; log_mean_w and ess within 1e-12 relative. Returns (list of failures, the numpy step, undecided count)."""
    st = step(pre_energy, beta_before, beta_end, rho, min_step)
    fails = []
    if abs(float(beta_after) - float(st["beta_next"])) > ulp32(st["beta_next"]):
        fails.append(f"beta_next {float(beta_after)!r} against {float(st['beta_next'])!r} ({st['by']})")
    db = float(np.float64(np.float32(beta_after)) - np.float64(np.float32(beta_before)))
    p = ha.plan(pre_energy, db, u)
    loose = int((p["margin"] <= ha.DECIDED).sum())
    if not loose and not np.array_equal(np.asarray(parent), p["parent"]):
        fails.append("parent")
    if st["F"]:
        if abs(log_mean_w - p["log_mean_w"]) > 1e-12 * max(abs(p["log_mean_w"]), np.finfo(float).tiny):
            fails.append(f"log_mean_w {log_mean_w!r} against {p['log_mean_w']!r}")
        if abs(ess - p["ess"]) > 1e-12 * p["ess"]:
            fails.append(f"ess {ess!r} against {p['ess']!r}")
    elif not (log_mean_w == -np.inf and ess == 0.0):
        fails.append("a deme without a finite energy")
    return fails, st, loose

"""The reference of population annealing (ppde_chains_set_annealing; tests/test_anneal_cpu.py, tests/test_anneal_gpu.py).

Annealing at inverse temperature beta IS reversible mode on the energy beta * E (helpers_tempering.ScaledEnergy on
helpers_reversible.reversible_iteration, as tempering's reference). What is new is the selection, restated here from
include/ppde_hip.h in fp64 numpy:

    demes of D chains with consecutive global indices; event behind iteration it when (it + 1) % every == 0 and
    s = (it + 1) / every - 1 < S; e_i the post-accept fp32 energies, dbeta = beta[s+1] - beta[s] in fp64;
    w_i = exp(dbeta (e_i - E_max)), 0 for a non-finite e_i; C = cumsum(w); W = C[-1];
    u = (Philox(first chain of the deme, it, 0x40000001, 0).x >> 8) * 2^-24; tau_j = (j + u) (W / D);
    a_j = #{i : C_i <= tau_j} clamped to the last i with w_i > 0; n_i = #{j : a_j = i};
    survivors keep their slot; the dead slots, in increasing order, take the surplus list (every i increasing, n_i - 1 times)."""
import itertools

import numpy as np
import torch

import helpers_reversible as hr
import helpers_tempering as ht
import ppde_oracle as orc
from ppde_amd import library as dl

SELECT_STREAM = 0x40000001
DECIDED = 1e-9                   # an offspring is decided when |tau_j - C_i| > DECIDED * W for every i
FAULTS = ("sign", "beta", "reverse", "history")


def select_uniforms(seed, first_chain, it):
    """u fp32 [len(first_chain)]: the selection uniform of every deme at iteration `it`."""
    first_chain = np.asarray(first_chain, dtype=np.uint32).reshape(-1)
    k = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint32)
    ctr = np.zeros((first_chain.size, 4), dtype=np.uint32)
    ctr[:, 0] = first_chain; ctr[:, 1] = it; ctr[:, 2] = SELECT_STREAM
    return (orc.philox4x32(ctr, k)[:, 0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def stage_of(it, every, S):
    """Stage of the event behind iteration `it`, or None."""
    if (it + 1) % every:
        return None
    s = (it + 1) // every - 1
    return s if s < S else None


def events_cap(S, max_steps, every):
    return min(S, max_steps // every)


def slots_of(counts, reverse=False):
    """parent [D] of the slot rule for offspring counts [D]. `reverse` plants a fault: the surplus list handed out backwards."""
    counts = np.asarray(counts)
    parent = np.arange(counts.size)
    dead = np.flatnonzero(counts == 0)
    surplus = np.repeat(np.arange(counts.size), np.maximum(counts - 1, 0))
    assert dead.size == surplus.size
    parent[dead] = surplus[::-1] if reverse else surplus
    return parent


def plan(e, dbeta, u, fault=None):
    """The plan of one deme: e fp32 [D] (what the device records as pre_energy), dbeta a Python / fp64 number, u the uniform.
    Returns dict(w, C, W, tau, anc [D], counts [D], parent [D], log_mean_w, ess, margin [D] = min_i |tau_j - C_i| / W)."""
    e32 = np.asarray(e, dtype=np.float32)
    D = e32.size
    fin = np.isfinite(e32)
    ident = dict(w=np.zeros(D), C=np.zeros(D), W=0.0, tau=np.zeros(D), anc=np.arange(D), counts=np.ones(D, np.int64),
                 parent=np.arange(D), log_mean_w=-np.inf, ess=0.0, margin=np.full(D, np.inf))
    if not fin.any():
        return ident
    db = -float(dbeta) if fault == "sign" else float(dbeta)
    ed = e32.astype(np.float64)
    emax = ed[fin].max() if fault != "sign" else ed[fin].min()            # (the flipped weights are largest at the LOWEST energy)
    w = np.zeros(D)
    w[fin] = np.exp(db * (ed[fin] - emax))
    C = np.cumsum(w)
    W = C[-1]
    tau = (np.arange(D) + float(u)) * (W / D)
    last = int(np.flatnonzero(w > 0)[-1])
    anc = np.minimum((C[None, :] <= tau[:, None]).sum(1), last)
    counts = np.bincount(anc, minlength=D)
    margin = np.abs(tau[:, None] - C[None, :]).min(1) / W
    return dict(w=w, C=C, W=W, tau=tau, anc=anc, counts=counts, parent=slots_of(counts, reverse=fault == "reverse"),
                log_mean_w=float(np.log(W / D) + db * emax), ess=float(W * W / (w * w).sum()), margin=margin)


def annealed_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length, nmut_threshold, betas, every, deme,
                 seed=0, chain_offset=0, allowed=None, trace=False, select_u=None, fault=None, keep_probs=False, forbidden=None,
                 motif_fault=None):
    """The whole mode on explicit noise: what hr.reversible_run returns (histories and best states on the UNTEMPERED energy;
    history row it + 1 and states[it + 1] describe the population AFTER selection), plus parent int32 [events, n] (local
    indices), pre_energy fp32 [events, n], log_mean_w / ess fp64 [events, n / D], beta fp32 [n] at the end, accepted
    [T, n] (the slots' own Metropolis results), post_accept (states, energies) per iteration, and select_margin, the smallest
    |tau_j - C_i| / W over all offspring. `select_u`: callable it -> u [n / D] replacing Philox. `keep_probs`: the traces keep the
    forward proposal rows (helpers_reversible.replay_margins reads them).
    `forbidden` = (patterns, allow_native): the iteration runs through helpers_motifs' constrained iteration on the
    same beta-scaled energy object, and the result gains vetoes int64 [n, M] (`motif_fault`: one of helpers_motifs' faults)."""
    betas = np.asarray(betas, dtype=np.float32)
    S, D = int(betas.size) - 1, int(deme)
    thr = hr._threshold(nmut_threshold)
    idx0 = torch.as_tensor(idx0).long()
    wt_idx = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    n, L = idx0.shape
    assert n % D == 0 and chain_offset % D == 0
    if allowed is None:
        allowed = dl.full_library(L)
    first = chain_offset + np.arange(n // D) * D
    beta = np.full(n, betas[0], np.float32)
    e0, f0 = energy.energy(idx0)
    e_hist, f_hist, states, accs, traces = [e0], [f0], [idx0.clone()], [], []
    best_e, best_f, best_t, best_x = e0.clone(), f0.clone(), torch.zeros(n, dtype=torch.long), idx0.clone()
    parents, pres, lmws, esss, post = [], [], [], [], []
    cur = idx0.clone()
    margin = np.inf
    import helpers_motifs as hmot
    iteration, con = hmot.iteration_of(forbidden, n, motif_fault)
    for it in range(num_steps):
        U, q, u = noise(it)
        sc = ht.ScaledEnergy(energy, beta)
        out = iteration(sc, cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=keep_probs)
        (ex, fx), (ey, fy) = sc.raw
        a = out["accepted"]
        cur = out["idx"].clone()
        e_new, f_new = torch.where(a, ey, ex).clone(), torch.where(a, fy, fx).clone()
        accs.append(a)
        if trace:
            traces.append(out)
        post.append((cur.clone(), e_new.clone()))

        def take_best(e_row, f_row, x_rows):
            better = e_row > best_e                                          # strict: the accept phase's rule
            best_e[better] = e_row[better]; best_f[better] = f_row[better]; best_t[better] = it + 1
            best_x[better] = x_rows[better]

        take_best(e_new, f_new, cur)
        s = stage_of(it, every, S)
        if s is not None:
            us = select_u(it) if select_u is not None else select_uniforms(seed, first, it)
            db = float(np.float64(betas[s + 1]) - np.float64(betas[s]))
            par = np.arange(n)
            lm, es = [], []
            en = e_new.numpy().copy()
            for d in range(n // D):
                p = plan(en[d * D:(d + 1) * D], db, us[d], fault=fault)
                par[d * D:(d + 1) * D] = d * D + p["parent"]
                lm.append(p["log_mean_w"]); es.append(p["ess"])
                margin = min(margin, float(p["margin"].min()))
            parents.append(par.astype(np.int32)); pres.append(en); lmws.append(lm); esss.append(es)
            pt = torch.as_tensor(par)
            cur = cur[pt].clone()
            if fault != "history":
                e_new, f_new = e_new[pt].clone(), f_new[pt].clone()
            take_best(e_new, f_new, cur)
            if fault != "beta":
                beta = np.full(n, betas[s + 1], np.float32)
        e_hist.append(e_new); f_hist.append(f_new); states.append(cur.clone())
    e_hist, f_hist, states = torch.stack(e_hist, 0), torch.stack(f_hist, 0), torch.stack(states, 0)
    E = len(parents)
    res = dict(best_idx=best_x, best_energy=best_e, best_fitness=best_f, best_step=best_t, energy_history=e_hist,
               fitness_history=f_hist, states=states,
               accepted=torch.stack(accs, 0) if accs else torch.zeros(0, n, dtype=torch.bool), final_idx=cur,
               parent=np.stack(parents, 0) if E else np.zeros((0, n), np.int32),
               pre_energy=np.stack(pres, 0) if E else np.zeros((0, n), np.float32),
               log_mean_w=np.array(lmws, np.float64).reshape(E, n // D), ess=np.array(esss, np.float64).reshape(E, n // D),
               beta=beta.copy(), post_accept=post, select_margin=margin)
    if trace:
        res["traces"] = traces
    if con is not None:
        res.update(vetoes=con.vetoes, veto_log=con.log)
    return res


# ------------------------------------------------------------------------------------------------ the exact selection matrix
def selection_matrix(E, dbeta, D, fault=None):
    """P_sel over slot-ordered joint states (x_0, ..., x_{D-1}) (index sum_i x_i S^(D-1-i)): row x holds the probability of
    every population the selection makes of x, from the fp32 energies `E` [S] by the plan above. The plan depends on u only
    through which side of the breakpoints u = C_i D / W - j it lies on, so the outcome is constant between consecutive
    breakpoints and its probability is the interval's length (the device's u lies on a 2^-24 lattice: 6e-8 per breakpoint,
    nothing a sample of 2^16 sees). `fault` plants 'sign' or 'reverse' (the others do not touch this matrix)."""
    E32 = np.asarray(E, dtype=np.float32)
    S = E32.size
    J = S ** D
    grid = np.stack(np.unravel_index(np.arange(J), (S,) * D), 1)
    P = np.zeros((J, J))
    for x in range(J):
        e = E32[grid[x]]
        p0 = plan(e, dbeta, 0.5, fault=fault if fault in ("sign", "reverse") else None)
        cuts = (p0["C"][None, :] * D / p0["W"] - np.arange(D)[:, None]).reshape(-1)
        cuts = np.unique(np.concatenate([[0.0, 1.0], cuts[(cuts > 0) & (cuts < 1)]]))
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p = plan(e, dbeta, 0.5 * (lo + hi), fault=fault if fault in ("sign", "reverse") else None)
            y = int(np.ravel_multi_index(tuple(grid[x][p["parent"]]), (S,) * D))
            P[x, y] += hi - lo
    return P


def kron_power(K, D):
    out = K
    for _ in range(D - 1):
        out = np.kron(out, K)
    return out


def joint_law_annealed(T, Ks, E, betas, every, D, start, fault=None, cache=None):
    """Row `start` (a joint index over slot-ordered states) of the product of the joint kernels of iterations 0 .. T - 1 of one
    deme: kron_D K_{beta now}, then the selection matrix of the stage behind an event. Ks: one enumerated reversible kernel per
    entry of the schedule (helpers_tempering.kernels_of(case, betas, pas)). 'history' leaves the law of the STATES alone.
    `cache`: a dict that keeps the joint kernels and selection matrices of one (Ks, E, betas, D) between calls."""
    betas = np.asarray(betas, dtype=np.float32)
    S_stages = betas.size - 1
    cache = {} if cache is None else cache
    joint, sel = cache.setdefault("joint", {}), cache.setdefault("sel", {})
    v = np.zeros(Ks[0].shape[0] ** D)
    v[start] = 1.0
    k = 0                                                                    # index of the beta the chains hold
    for it in range(T):
        if k not in joint:
            joint[k] = kron_power(Ks[k], D)
        v = v @ joint[k]
        s = stage_of(it, every, S_stages)
        if s is not None:
            key = (s, fault if fault in ("sign", "reverse") else None)
            if key not in sel:
                sel[key] = selection_matrix(E, float(np.float64(betas[s + 1]) - np.float64(betas[s])), D, key[1])
            v = v @ sel[key]
            if fault != "beta":
                k = s + 1
    return v


def deme_cells(idx, D, allowed, index, start_row, S):
    """Joint cell of every deme of a population idx [n, L]: (cells [n / D], forbidden)."""
    import helpers_library as hl
    cells, forbidden = hl.state_cells(idx, allowed, index, start_row)
    return np.ravel_multi_index(tuple(cells.reshape(-1, D).T), (S,) * D), forbidden


# ------------------------------------------------------------------------------------------------ the cases
REPLAY_BETAS = (0.25, 0.5, 1.0)           # powers of two: scaling commutes with the rounding (helpers_tempering's argument)
REPLAY = dict(n=12, T=9, pas=2, nmut=3, philox_seed=233)
LAW_BETAS_A = (0.5, 1.0)                  # case A, D = 2: one stage
LAW_BETAS_B = (0.25, 0.5, 1.0)            # case B, D = 3 and 4: two stages
LAW_T = (1, 2, 3, 8)
LAW_EVERY = (1, 2)
# joint start states (slot 0, slot 1, ...) from which the law tests see the planted faults (tests/test_anneal_cpu.py says which
# fault each case can see: handing the surplus out backwards changes nothing below four slots)
POWER_START_A = (32, 20)
POWER_START_B = {3: (3, 4, 3), 4: (4, 0, 0, 1)}


def founders_by_hand():
    """A hand-made genealogy of 2 demes of 3 over 2 events, with what anneal.summarise must say of it."""
    parent = np.array([[0, 0, 2, 3, 4, 4], [2, 1, 2, 3, 3, 3]])
    log_mean_w = np.array([[0.5, -0.25], [0.125, 1.0]])
    ess = np.array([[2.0, 2.5], [1.5, 1.0]])
    expect = dict(log_z_ratio=np.array([0.625, 0.75]), founders_alive=np.array([[2, 2], [2, 1]]), replaced=np.array([2, 3]),
                  ess_min=np.array([2.0, 1.0]))
    return parent, log_mean_w, ess, expect

"""The reference of reversible mode (ppde_chains_set_reversible; tests/test_reversible_cpu.py, tests/test_reversible_gpu.py).

Nothing under oracle/ knows this mode: it is built here from the oracle's own fp32 functions (`orc.forward_logits`,
`orc.race_sample`, `orc.log_prob_at`) on explicit noise. One function forms every proposal row,

    row(g, state):  z = forward_logits(g, state)              range mask and the cap mask OF THAT STATE as -inf
                    z[l, k] = -inf where the library forbids (l, k)
                    p = clamp(softmax(z - logsumexp z), 2^-23, 1 - 2^-23);  p = 0 where forbidden;  p_hat = p / sum(p)

(the forward row exactly as helpers_library.masked_oracle forms it), and an iteration is a Metropolis-Hastings step of the
path proposal built from it: forward rows row(g_x, x_s) as before; the reverse row of sub-step s is row(g_y, x_{s+1}) read at
the move that UNDOES the sub-step, (l_s, old_s) with old_s the letter residue l_s held in x_s; a path with a reverse move of
probability exactly 0 (forbidden by the library, or a reverse row with no admissible entry) is rejected; a proposal with
dist(y) >= nmut_threshold is rejected; nothing is ever reset to the wild type."""
import itertools
import math

import numpy as np
import torch

import ppde_oracle as orc
from ppde_amd import library as dl

A = 20


def _threshold(nmut_threshold):
    return np.iinfo(np.int32).max if nmut_threshold == 0 else int(nmut_threshold)


def proposal_row(grad, state, wt_idx, min_pos, max_pos, thr, forbid):
    """row(g, state) for all chains: p_hat fp32 [n, L*A], and which rows have no admissible entry at all."""
    z = orc.forward_logits(grad, state, wt_idx, min_pos, max_pos, thr)
    z = torch.where(forbid, torch.tensor(-math.inf), z)
    dead = torch.isinf(z).all(-1)
    z = torch.where(dead.reshape(-1, 1), torch.zeros(()), z)              # (placeholder row: such a path is rejected)
    z = z - torch.logsumexp(z, dim=-1, keepdim=True)
    p = torch.softmax(z, dim=-1).clamp(min=orc.EPS, max=1.0 - orc.EPS)
    p = torch.where(forbid, torch.tensor(0.0), p)
    return p / p.sum(-1, keepdim=True), dead


def reversible_iteration(energy, idx_cur, idx_reject, wt_idx, U, q, u, min_pos, max_pos, nmut_threshold, allowed,
                         keep_probs=False):
    """One reversible iteration for all chains: arguments and returned dict as orc.pas_iteration's, plus `allowed` (uint32 [L] or
    bool [L, 20]). `nmut_threshold` is the threshold itself (int32 max = none), as orc.pas_iteration takes it. Extra keys:
    `undo` [max_u, n] the flat indices the reverse rows are read at, `refused` [n] the proposals the rule rejects whatever u
    is (a forbidden reverse move, or the cap)."""
    n, L = idx_cur.shape
    thr = int(nmut_threshold)
    forbid = torch.as_tensor(~dl.as_bool(allowed)).reshape(1, -1)
    max_u = int(U.max())
    ar = torch.arange(n)
    e_x, fit_x, g_x = energy.energy_grad(idx_cur)
    cur = idx_cur.clone()
    flats, undo, logp_fwd, after, p_fwd = [], [], [], [], []
    for s in range(max_u):
        p_hat, _ = proposal_row(g_x, cur, wt_idx, min_pos, max_pos, thr, forbid)
        if keep_probs:
            p_fwd.append(p_hat)
        flat = orc.race_sample(p_hat, q[s])
        flats.append(flat)
        logp_fwd.append(orc.log_prob_at(p_hat, flat))
        undo.append((flat // A) * A + cur[ar, flat // A])                    # restores the letter this sub-step replaces
        active = s < U
        nxt = cur.clone()
        nxt[ar, flat // A] = flat % A
        cur = torch.where(active.reshape(n, 1), nxt, cur)
        after.append(cur.clone())
    e_y, fit_y, g_y = energy.energy_grad(cur)
    log_ratio = torch.zeros(n)
    refused = torch.zeros(n, dtype=torch.bool)
    logp_rev = []
    for s in range(max_u):
        p_rev, dead = proposal_row(g_y, after[s], wt_idx, min_pos, max_pos, thr, forbid)
        lr = orc.log_prob_at(p_rev, undo[s])
        logp_rev.append(lr)
        active = s < U
        refused |= active & (dead | (p_rev.gather(1, undo[s].reshape(-1, 1)).reshape(-1) == 0))
        log_ratio = log_ratio + active.float() * (lr - logp_fwd[s])
    log_acc = (e_y - e_x) + log_ratio
    refused |= (cur != wt_idx.reshape(1, L)).sum(-1) >= thr                   # the cap is a constraint of the target
    acc = (torch.exp(log_acc) >= u) & ~refused
    out = dict(idx=torch.where(acc.reshape(n, 1), cur, idx_reject), energy=torch.where(acc, e_y, e_x),
               fitness=torch.where(acc, fit_y, fit_x), accepted=acc, log_acc=log_acc, flat=torch.stack(flats, 0), proposal=cur,
               logp_fwd=torch.stack(logp_fwd, 0), logp_rev=torch.stack(logp_rev, 0), undo=torch.stack(undo, 0), refused=refused,
               e_x=e_x, e_y=e_y, fit_x=fit_x, fit_y=fit_y, grad_x=g_x, grad_y=g_y)
    if keep_probs:
        out["p_fwd"] = torch.stack(p_fwd, 0)
    return out


def reversible_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length=2, nmut_threshold=0,
                   paper_results=False, trace=False, record_after_reset=False, keep_probs=False, allowed=None):
    """The whole sampler in reversible mode on explicit noise: arguments and returned dict as orc.run's, plus `allowed`
    (None = every letter everywhere). There is no reset, so `record_after_reset` changes nothing; `paper_results` is refused."""
    if paper_results:
        raise ValueError("reversible mode: paper_results restarts a rejected chain from its initial state, which is no Metropolis step")
    thr = _threshold(nmut_threshold)
    idx0 = torch.as_tensor(idx0).long()
    wt_idx = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    n, L = idx0.shape
    if allowed is None:
        allowed = dl.full_library(L)
    e0, f0 = energy.energy(idx0)
    e_hist, f_hist, states, accs, traces = [e0], [f0], [idx0.clone()], [], []
    cur = idx0.clone()
    for it in range(num_steps):
        U, q, u = noise(it)
        out = reversible_iteration(energy, cur, cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=keep_probs)
        cur = out["idx"].clone()
        e_hist.append(out["energy"])
        f_hist.append(out["fitness"])
        accs.append(out["accepted"])
        if trace:
            traces.append(out)
        states.append(cur.clone())
    e_hist, f_hist, states = torch.stack(e_hist, 0), torch.stack(f_hist, 0), torch.stack(states, 0)
    best_e, best_t = torch.max(e_hist, 0)                                     # first index on ties
    ar = torch.arange(n)
    res = dict(best_idx=states[best_t, ar], best_energy=best_e, best_fitness=f_hist[best_t, ar], energy_history=e_hist,
               fitness_history=f_hist, states=states,
               accepted=torch.stack(accs, 0) if accs else torch.zeros(0, n, dtype=torch.bool), final_idx=cur)
    if trace:
        res["traces"] = traces
    return res


def exact_reversible_kernel(energy, wt_idx, allowed, pas_length, min_pos, max_pos, nmut_threshold=0):
    """The Markov kernel of ONE reversible iteration as an explicit matrix, enumerated over what
    helpers_library.exact_library_kernel enumerates: states = every combination of allowed letters at the open residues (all
    other residues wild type), paths = every sequence of allowed moves of every length 1 .. 2 pas - 1. Every open residue must
    lie inside [min_pos, max_pos]. A path never leaves that state space, so every row a path can meet is one of
    row(g_a, state_b): they are formed ONCE, by `proposal_row` in fp32, their log-probabilities as orc.log_prob_at forms them,
    and a path's weight and log-ratio are then read from these tables -- the products in fp64, the log-ratio summed in fp32 in
    reversible_iteration's order; the diagonal is the complement of the accepted flows to other states, so rows sum to 1
    exactly. (tests/test_reversible_cpu.py holds the result against reversible_run's own sampling.)
    Returns (K float64 [S, S], states int64 [S, L], index dict: tuple of the open residues' letters -> row, energies float64
    [S], inside bool [S]: the states with dist < nmut_threshold -- the support of the stationary law. Only the rows of those
    states are enumerated: no state inside ever moves outside, so the rows of the others are never needed and stay zero)."""
    wt = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    L = wt.numel()
    ok = dl.as_bool(allowed)
    positions = [int(p) for p in np.flatnonzero(ok.any(1))]
    assert positions and min_pos <= positions[0] and positions[-1] <= max_pos, "open residues must lie inside the range"
    thr = _threshold(nmut_threshold)
    forbid = torch.as_tensor(~ok).reshape(1, -1)
    choices = [list(np.flatnonzero(ok[p])) for p in positions]
    combos = list(itertools.product(*choices))
    index = {tuple(int(v) for v in c): i for i, c in enumerate(combos)}
    S = len(combos)
    states = wt.repeat(S, 1)
    states[:, positions] = torch.as_tensor(np.array(combos, dtype=np.int64))
    moves = np.array([p * A + k for p, ch in zip(positions, choices) for k in ch], dtype=np.int64)
    M = len(moves)
    move_of = {int(f): j for j, f in enumerate(moves)}
    inside = ((states != wt.reshape(1, L)).sum(-1) < thr).numpy()
    e32, _, grad = energy.energy_grad(states)
    # tables over (gradient of an inside state, state, move): probability, log-probability, rows without an admissible entry
    G = np.flatnonzero(inside)
    g_of = np.full(S, -1)
    g_of[G] = np.arange(len(G))
    cols = torch.as_tensor(moves)
    P = np.zeros((len(G), S, M), np.float32)
    LP = np.zeros((len(G), S, M), np.float32)
    dead = np.zeros((len(G), S), bool)
    for gi, x in enumerate(G):
        p_hat, d = proposal_row(grad[x:x + 1].expand(S, L, A), states, wt, min_pos, max_pos, thr, forbid)
        P[gi] = p_hat[:, cols].numpy()
        LP[gi] = torch.log(p_hat.clamp(min=orc.EPS, max=1.0 - orc.EPS))[:, cols].numpy()           # orc.log_prob_at's formula
        dead[gi] = d.numpy()
    # where a move leads, and the move that undoes it
    st = states.numpy()
    nxt = np.zeros((S, M), np.int64)
    undo = np.zeros((S, M), np.int64)
    for j, f in enumerate(moves):
        l, k = int(f) // A, int(f) % A
        moved = st.copy()
        moved[:, l] = k
        nxt[:, j] = [index[tuple(int(v) for v in row)] for row in moved[:, positions]]
        undo[:, j] = [move_of[l * A + int(v)] for v in st[:, l]]
    e_np = e32.numpy()
    K = np.zeros((S, S))
    n_len = 2 * pas_length - 1
    for x in G:
        xi = g_of[x]
        for U in range(1, n_len + 1):
            paths = np.array(list(itertools.product(range(M), repeat=U)), dtype=np.int64)
            c = paths.shape[0]
            s_cur = np.full(c, x)
            p_path = np.ones(c)
            lpf, und, after = [], [], []
            for s in range(U):
                m = paths[:, s]
                p_path = p_path * P[xi, s_cur, m].astype(np.float64)
                lpf.append(LP[xi, s_cur, m])
                und.append(undo[s_cur, m])
                s_cur = nxt[s_cur, m]
                after.append(s_cur)
            y = s_cur
            refused = ~inside[y]                                              # the cap is a constraint of the target
            yi = np.where(inside[y], g_of[y], 0)
            log_ratio = np.zeros(c, np.float32)
            for s in range(U):
                refused |= dead[yi, after[s]] | (P[yi, after[s], und[s]] == 0)
                log_ratio = log_ratio + (LP[yi, after[s], und[s]] - lpf[s])
            log_acc = (e_np[y] - e_np[x]) + log_ratio
            with np.errstate(over="ignore"):
                a = np.minimum(1.0, np.exp(log_acc.astype(np.float64)))
            a[refused] = 0.0
            w = p_path / n_len
            np.add.at(K[x], y, w * a)
        # what is not accepted elsewhere stays: the diagonal is the complement of the off-diagonal flows, so every enumerated row
        # is a distribution to fp64 rounding (summing the fp32 path probabilities' rejected parts instead leaves rows that miss
        # 1 by ~2e-7, which a power of K compounds)
        K[x, x] = 0.0
        K[x, x] = 1.0 - K[x].sum()
    return K, states, index, e32.double().numpy(), inside


def target_law(energies, inside):
    """exp(E) * 1[inside] / Z in fp64."""
    w = np.where(inside, np.exp(energies - energies[inside].max()), 0.0)
    return w / w.sum()


def detailed_balance_residual(K, pi):
    """Worst |pi_x K_xy - pi_y K_yx| / max(pi_x K_xy, pi_y K_yx) over the pairs x != y with a positive flow either way."""
    F = pi[:, None] * K
    big = np.maximum(F, F.T)
    off = ~np.eye(K.shape[0], dtype=bool) & (big > 0)
    return float((np.abs(F - F.T)[off] / big[off]).max())


def stationary_vector(K):
    """The stationary vector of a row-stochastic K (fp64 null vector of K^T - I, normalised)."""
    S = K.shape[0]
    M = np.vstack([K.T - np.eye(S), np.ones((1, S))])
    rhs = np.zeros(S + 1)
    rhs[-1] = 1.0
    return np.linalg.lstsq(M, rhs, rcond=None)[0]


def total_variation(p, q):
    return 0.5 * float(np.abs(np.asarray(p) - np.asarray(q)).sum())


def cap_case(seed=57):
    """The cap case of the law tests: L = 7, Potts window 0..5, residues 2 and 3 open with 11 letters each, to be run with
    nmut_threshold 2 (at most one mutation): 1 + 10 + 10 = 21 states inside the cap out of 121."""
    from ppde_amd import synthetic
    L, Lp, i0 = 7, 6, 0
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, sigma_J=0.3, sigma_h=0.8)
    allowed = np.zeros(L, np.uint32)
    for site, count in ((2, 11), (3, 11)):
        others = [k for k in rng.permutation(A).tolist() if k != int(wt[site])][:count - 1]
        allowed[site] = sum(1 << k for k in others) | (1 << int(wt[site]))
    return dict(L=L, Lp=Lp, i0=i0, wt=wt, J=J, h=h, allowed=allowed, cnn=None, lamda=0.0, nmut=2)


# ------------------------------------------------------------------------------------------------ the replay cases
# TOY24, Potts + CNN, helpers_library.seeded_library(seed 41), chains from the wild type. `torch_seed` seeds the noise of the
# flat-race replay (rng_mode 0, T iterations), `philox_seed` is the device RNG's key (rng_mode 1, T_dev iterations: the shortest
# run a graph segment fits). The seeds were picked so that no accept
# decision and no race of the REFERENCE comes closer to a tie than tests/test_reversible_cpu.py's margins.
REPLAY_CASES = {
    "pas2": dict(n=16, T=12, T_dev=20, pas=2, nmut=0, torch_seed=2111, philox_seed=99),
    "pas2_cap3": dict(n=16, T=12, T_dev=20, pas=2, nmut=3, torch_seed=2103, philox_seed=103),
    "pas3": dict(n=16, T=8, T_dev=20, pas=3, nmut=0, torch_seed=2105, philox_seed=99),
    # set_reversible without set_library: the range mask alone, whose entries keep the 2^-23 floor in both directions
    "pas2_nolib": dict(n=16, T=12, T_dev=20, pas=2, nmut=3, torch_seed=2117, philox_seed=99, library=False),
}


def replay_model():
    import helpers_library as hl
    c = hl.toy24()
    lib = hl.seeded_library(c["wt"], c["i0"], c["i0"] + c["Lp"] - 1, seed=41)
    return c, lib


def replay_noise(name, rng_mode, L):
    """The noise of replay case `name`: torch's generator in the reference's order (rng_mode 0, flat race) or the device RNG's
    draws restated on the CPU (rng_mode 1, two-level draw; orc.device_noise)."""
    k = REPLAY_CASES[name]
    if rng_mode == 0:
        gen = torch.Generator().manual_seed(k["torch_seed"])
        return [orc.draw_noise_torch(k["n"], L * A, k["pas"], generator=gen) for _ in range(k["T"])]
    return [orc.device_noise(k["philox_seed"], 0, k["n"], t, k["pas"], L) for t in range(k["T_dev"])]


def replay_reference(name, rng_mode, energy, c, lib, keep_probs=False):
    k = REPLAY_CASES[name]
    if not k.get("library", True):
        lib = None
    noise = replay_noise(name, rng_mode, c["L"])
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    ref = reversible_run(energy, np.tile(c["wt"].astype(np.int64), (k["n"], 1)), c["wt"], lambda t: noise[t], len(noise), lo, hi,
                         k["pas"], k["nmut"], trace=True, keep_probs=keep_probs, allowed=lib)
    return noise, ref


def replay_margins(noise, ref):
    """(smallest |log_acc - log u| over the decisions u takes, smallest race gap against the runner-up) of a reference run."""
    acc_margin, gap = math.inf, math.inf
    for t, out in enumerate(ref["traces"]):
        U, q, u = noise[t]
        free = ~out["refused"]
        d = (out["log_acc"] - torch.log(u)).abs()[free]
        if d.numel():
            acc_margin = min(acc_margin, float(d.min()))
        for s in range(int(U.max())):
            for b in np.flatnonzero((s < U).numpy()):
                p, qq, win = out["p_fwd"][s, b], q[s, b], int(out["flat"][s, b])
                N = p.shape[-1]
                if qq.shape[-1] == N:
                    v = p / qq
                    v[win] = -1.0
                    gap = min(gap, orc.race_gap(p, qq, int(torch.argmax(v))))
                else:
                    L = N // A
                    pl = p.reshape(L, A)
                    vres = pl.sum(-1) / qq[:L]
                    vres[win // A] = -1.0
                    if float(vres.max()) > 0:
                        gap = min(gap, orc.race_gap(p, qq, int(torch.argmax(vres)) * A + win % A))
                    vlet = pl[win // A] / qq[L:]
                    vlet[win % A] = -1.0
                    if float(vlet.max()) > 0:
                        gap = min(gap, orc.race_gap(p, qq, (win // A) * A + int(torch.argmax(vlet))))
    return acc_margin, gap

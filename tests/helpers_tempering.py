"""The reference of parallel tempering (ppde_chains_set_tempering; tests/test_tempering_cpu.py, tests/test_tempering_gpu.py).

Tempering at inverse temperature beta IS reversible mode on the energy beta * E, so nothing new has to be trusted for the chain
kernels: `ScaledEnergy` hands (beta e, beta fit, beta g) to helpers_reversible's own `reversible_iteration` and
`exact_reversible_kernel`. What is new is the replica exchange, restated here from include/ppde_hip.h:

    ensembles of R chains with consecutive global indices, chain g starts on rung g % R;
    swap event after the accept phase of iteration it when swap_every > 0 and (it + 1) % swap_every == 0, event number
    s = (it + 1) / swap_every - 1; rungs (r, r + 1) with r = s (mod 2), r + 1 < R are paired;
    a = chain on rung r, b = chain on rung r + 1:  d = (beta_r - beta_{r+1}) * (E_b - E_a)  in fp32 on the untempered
    post-accept energies, accepted when exp(d) >= u, u = (Philox(first chain of the ensemble, it, 0x40000000, r).x >> 8) * 2^-24;
    a swap exchanges temperatures (beta, rung, the rung -> chain map), never states."""
import numpy as np
import torch

import helpers_reversible as hr
import ppde_oracle as orc
from ppde_amd import library as dl
from ppde_amd import synthetic

A = 20
SWAP_STREAM = 0x40000000


class ScaledEnergy:
    """energy -> (beta e, beta fit, beta g); beta a float or fp32 [n] (one per chain). The unscaled (e, fit) of the calls so
    far are kept in `raw`, in call order: what the histories of a tempering run hold."""

    def __init__(self, energy, beta):
        self.energy_fn = energy
        self.beta = torch.as_tensor(np.asarray(beta, dtype=np.float32))
        self.raw = []

    def energy(self, idx):
        e, f = self.energy_fn.energy(idx)
        self.raw.append((e, f))
        return self.beta * e, self.beta * f

    def energy_grad(self, idx):
        e, f, g = self.energy_fn.energy_grad(idx)
        self.raw.append((e, f))
        b = self.beta.reshape(-1, 1, 1) if self.beta.ndim else self.beta
        return self.beta * e, self.beta * f, b * g


def swap_uniforms(seed, first_chain, it, R):
    """u [len(first_chain), R]: the swap uniform of every (ensemble, lower rung r) at iteration `it`, restated from
    orc.philox4x32 and the accept uniform's conversion (orc.device_noise)."""
    first_chain = np.asarray(first_chain, dtype=np.uint32)
    k = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint32)
    ctr = np.zeros((first_chain.size, R, 4), dtype=np.uint32)
    ctr[..., 0] = first_chain[:, None]; ctr[..., 1] = it; ctr[..., 2] = SWAP_STREAM; ctr[..., 3] = np.arange(R)[None]
    return (orc.philox4x32(ctr, k)[..., 0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def swap_pairs(it, swap_every, R):
    """The lower rungs paired by the swap event behind iteration `it` (empty: no event, or no pair of that parity)."""
    if swap_every <= 0 or (it + 1) % swap_every:
        return []
    s = (it + 1) // swap_every - 1
    return [r for r in range(R - 1) if r % 2 == s % 2]


def swap_decision(beta_lo, beta_hi, e_a, e_b, u):
    """(accepted, d) of the swap rule in fp32: d = (beta_r - beta_{r+1}) * (E_b - E_a), accepted when exp(d) >= u."""
    d = (np.float32(beta_lo) - np.float32(beta_hi)) * (np.float32(e_b) - np.float32(e_a))
    with np.errstate(over="ignore"):
        return bool(np.exp(np.float32(d)) >= np.float32(u)), float(d)


def tempered_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length, nmut_threshold, betas, swap_every,
                 seed=0, chain_offset=0, allowed=None, trace=False, keep_probs=False, swap_u=None, forbidden=None, motif_fault=None):
    """The whole algorithm on explicit noise: what hr.reversible_run returns (histories and best states on the UNTEMPERED
    energy), plus rung_history uint8 [T+1, n], rung / beta [n] at the end, swap_attempts / swap_accepts int64 [n/R, R-1] and
    swap_margin, the smallest |d - log u| over the swap decisions. `swap_u`: callable it -> u [n/R, R] replacing Philox.
    `forbidden` = (patterns, allow_native): the iteration runs through helpers_motifs' constrained iteration on the
    same beta-scaled energy object, and the result gains vetoes int64 [n, M] (`motif_fault`: one of helpers_motifs' faults)."""
    betas = np.asarray(betas, dtype=np.float32)
    R = int(betas.size)
    thr = hr._threshold(nmut_threshold)
    idx0 = torch.as_tensor(idx0).long()
    wt_idx = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    n, L = idx0.shape
    assert n % R == 0 and chain_offset % R == 0
    if allowed is None:
        allowed = dl.full_library(L)
    n_ens = n // R
    rung = (np.arange(n) % R).astype(np.int32)
    beta = betas[rung].copy()
    slot = np.arange(n).reshape(n_ens, R).copy()
    att, acc_n = np.zeros((n_ens, R - 1), np.int64), np.zeros((n_ens, R - 1), np.int64)
    first = chain_offset + np.arange(n_ens) * R
    e0, f0 = energy.energy(idx0)
    e_hist, f_hist, states, accs, traces, rung_hist = [e0], [f0], [idx0.clone()], [], [], [rung.astype(np.uint8)]
    cur = idx0.clone()
    margin = np.inf
    import helpers_motifs as hmot
    iteration, con = hmot.iteration_of(forbidden, n, motif_fault)
    for it in range(num_steps):
        U, q, u = noise(it)
        sc = ScaledEnergy(energy, beta)
        out = iteration(sc, cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=keep_probs)
        (ex, fx), (ey, fy) = sc.raw
        a = out["accepted"]
        cur = out["idx"].clone()
        e_new, f_new = torch.where(a, ey, ex), torch.where(a, fy, fx)
        e_hist.append(e_new); f_hist.append(f_new); accs.append(a); states.append(cur.clone())
        if trace:
            traces.append(out)
        pairs = swap_pairs(it, swap_every, R)
        if pairs:
            us = swap_u(it) if swap_u is not None else swap_uniforms(seed, first, it, R)
            en = e_new.numpy()
            for e_i in range(n_ens):
                for r in pairs:
                    ca, cb = slot[e_i, r], slot[e_i, r + 1]
                    ok, d = swap_decision(beta[ca], beta[cb], en[ca], en[cb], us[e_i, r])
                    if us[e_i, r] > 0:
                        margin = min(margin, abs(d - float(np.log(np.float64(us[e_i, r])))))
                    att[e_i, r] += 1
                    if ok:
                        acc_n[e_i, r] += 1
                        beta[ca], beta[cb] = beta[cb], beta[ca]
                        rung[ca], rung[cb] = r + 1, r
                        slot[e_i, r], slot[e_i, r + 1] = cb, ca
        rung_hist.append(rung.astype(np.uint8))
    e_hist, f_hist, states = torch.stack(e_hist, 0), torch.stack(f_hist, 0), torch.stack(states, 0)
    best_e, best_t = torch.max(e_hist, 0)
    ar = torch.arange(n)
    res = dict(best_idx=states[best_t, ar], best_energy=best_e, best_fitness=f_hist[best_t, ar], energy_history=e_hist,
               fitness_history=f_hist, states=states,
               accepted=torch.stack(accs, 0) if accs else torch.zeros(0, n, dtype=torch.bool), final_idx=cur,
               rung_history=np.stack(rung_hist, 0), rung=rung.copy(), beta=beta.copy(), swap_attempts=att, swap_accepts=acc_n,
               swap_margin=margin)
    if trace:
        res["traces"] = traces
    if con is not None:
        res.update(vetoes=con.vetoes, veto_log=con.log)
    return res


def swap_matrix(E, betas, parity, fault=None):
    """P_swap over rung-ordered joint states (x_0, ..., x_{R-1}) (index sum_r x_r S^(R-1-r)): every pair (r, r + 1) with
    r = parity (mod 2) exchanges its two states with probability min(1, exp(d)), d from the rule in fp32 on the oracle's fp32
    energies `E` [S]. `fault` plants a wrong rule (power of the law tests): 'sign' reverses d, 'scaled' forms d from the
    beta-scaled energies ((beta_r - beta_{r+1}) (beta_{r+1} E_b - beta_r E_a)), 'parity' pairs every rung r with r + 1 taken two at a time from 0."""
    E32 = np.asarray(E, dtype=np.float32)
    b32 = np.asarray(betas, dtype=np.float32)
    S, R = E32.size, b32.size
    J = S ** R
    grid = np.stack(np.unravel_index(np.arange(J), (S,) * R), 1)
    P = np.eye(J)
    if parity is None:
        return P
    par = 0 if fault == "parity" else parity % 2
    for r in range(par, R - 1, 2):
        xa, xb = grid[:, r], grid[:, r + 1]
        if fault == "scaled":
            d = (b32[r] - b32[r + 1]) * (b32[r + 1] * E32[xb] - b32[r] * E32[xa])
        else:
            d = (b32[r] - b32[r + 1]) * (E32[xb] - E32[xa])
        if fault == "sign":
            d = -d
        with np.errstate(over="ignore"):
            a = np.minimum(1.0, np.exp(d.astype(np.float32)).astype(np.float64))
        sw = grid.copy()
        sw[:, r], sw[:, r + 1] = xb, xa
        j2 = np.ravel_multi_index(tuple(sw.T), (S,) * R)
        Pp = np.zeros((J, J))
        np.add.at(Pp, (np.arange(J), j2), a)
        np.add.at(Pp, (np.arange(J), np.arange(J)), 1.0 - a)
        P = P @ Pp
    return P


def exact_tempered_kernel(Ks, E, betas, parity, fault=None):
    """The joint kernel of one iteration of an ensemble, (kron_r K_{beta_r}) . P_swap, over rung-ordered joint states.
    `parity` None: an iteration without a swap event."""
    K = Ks[0]
    for Kr in Ks[1:]:
        K = np.kron(K, Kr)
    return K if parity is None else K @ swap_matrix(E, betas, parity, fault)


def joint_law(num_steps, Ks, E, betas, swap_every, start, fault=None):
    """Row `start` (a joint index) of the product of the joint kernels of iterations 0 .. num_steps - 1."""
    plain = exact_tempered_kernel(Ks, E, betas, None)
    swapped = {}
    v = np.zeros(plain.shape[0])
    v[start] = 1.0
    for it in range(num_steps):
        if swap_every > 0 and (it + 1) % swap_every == 0:
            par = ((it + 1) // swap_every - 1) % 2
            if par not in swapped:
                swapped[par] = exact_tempered_kernel(Ks, E, betas, par, fault)
            v = v @ swapped[par]
        else:
            v = v @ plain
    return v


def product_law(E, betas, inside=None):
    """prod_r exp(beta_r E(x_r)) / Z_r over rung-ordered joint states, fp64."""
    E = np.asarray(E, dtype=np.float64)
    inside = np.ones(E.size, bool) if inside is None else inside
    p = None
    for b in np.asarray(betas, dtype=np.float32).astype(np.float64):
        pr = hr.target_law(b * E, inside)
        p = pr if p is None else np.kron(p, pr)
    return p


def kernels_of(case, betas, pas):
    """(Ks, states, index, E fp64 [S] untempered, inside) of a law case: one enumerated reversible kernel per rung, on beta E."""
    import helpers_library as hl
    en = hl.oracle_energy_of(case)
    Ks, out = [], None
    for b in np.asarray(betas, dtype=np.float32):
        K, states, index, _, inside = hr.exact_reversible_kernel(ScaledEnergy(en, float(b)), case["wt"], case["allowed"], pas, 0,
                                                                 case["L"] - 1, case.get("nmut", 0))
        Ks.append(K)
        out = (states, index, inside)
    e32, _ = en.energy(out[0])
    return Ks, out[0], out[1], e32.double().numpy(), out[2]


def joint_cells(idx, rung, R, allowed, index, start_row, S):
    """Joint cell of every ensemble of a population idx [n, L] whose chains hold rungs `rung` [n]: (cells [n/R], forbidden)."""
    import helpers_library as hl
    cells, forbidden = hl.state_cells(idx, allowed, index, start_row)
    n = cells.size
    rung = np.asarray(rung).astype(np.int64).reshape(n // R, R)
    assert (np.sort(rung, 1) == np.arange(R)[None]).all(), "every ensemble holds every rung once"
    by_rung = np.take_along_axis(cells.reshape(n // R, R), np.argsort(rung, 1), 1)
    return np.ravel_multi_index(tuple(by_rung.T), (S,) * R), forbidden


def expected_pearson(p_true, p_fault, n, floor=8.0):
    """Expected Pearson statistic, df + n sum (p' - p)^2 / p over helpers_library.chi_square's pooled cells, of a sample of
    size n from `p_fault` tested against `p_true`; returns (statistic, df)."""
    e = n * p_true
    small = e < floor
    p = np.append(p_true[~small], p_true[small].sum())
    q = np.append(p_fault[~small], p_fault[small].sum())
    keep = p > 0
    p, q = p[keep], q[keep]
    df = len(p) - 1
    return float(df + n * ((q - p) ** 2 / p).sum()), df


def one_site_case(L, Lp, i0, site, letters=A, seed=31):
    """One open residue with `letters` letters (wild type included), Potts only: tests/test_reversible_gpu.py's geometries."""
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed, sigma_J=0.3, sigma_h=0.8)
    allowed = np.zeros(L, np.uint32)
    others = [k for k in rng.permutation(A).tolist() if k != int(wt[site])][:letters - 1]
    allowed[site] = sum(1 << k for k in others) | (1 << int(wt[site]))
    return dict(L=L, Lp=Lp, i0=i0, wt=wt, J=J, h=h, allowed=allowed, cnn=None, lamda=0.0, nmut=0)


def case_a():
    import helpers_library as hl
    return dict(hl.law_case(), cnn=None, lamda=0.0, nmut=0)


def case_b():
    return one_site_case(8, 6, 1, 4, letters=5)


BETAS_A = (1.0, 0.5)
POWER_START_A = (17, 3)           # joint start state (rung 0, rung 1) from which the law tests can see every planted swap fault
BETAS_B = (1.0, 0.5, 0.25, 0.125)
SWAP_EVERY_B = 2

# ------------------------------------------------------------------------------------------------ the replay cases
# helpers_reversible's TOY24 cases under the ladder (1, 1/2, 1/4, 1/8): powers of two commute with the rounding, so the device's
# beta * ((g - g_cur) / 2) and the reference's (beta g - beta g_cur) / 2 are the same fp32 numbers. Seeds picked so that no
# accept decision, race or swap decision of the REFERENCE comes closer to a tie than tests/test_tempering_cpu.py demands.
REPLAY_BETAS = (1.0, 0.5, 0.25, 0.125)
REPLAY_CASES = {
    "pas2": dict(n=16, T=12, T_dev=20, pas=2, nmut=0, torch_seed=2203, philox_seed=233),
    "pas2_cap3": dict(n=16, T=12, T_dev=20, pas=2, nmut=3, torch_seed=2201, philox_seed=202),
    "pas3": dict(n=16, T=8, T_dev=20, pas=3, nmut=0, torch_seed=2203, philox_seed=216),
}
REPLAY_SWAPS = (0, 1, 3)          # swap_every of the device-RNG replays; the flat-race replay runs 0 only
T_DEV_LONG = 40


def replay_noise(name, rng_mode, L, T=None):
    k = REPLAY_CASES[name]
    if rng_mode == 0:
        gen = torch.Generator().manual_seed(k["torch_seed"])
        return [orc.draw_noise_torch(k["n"], L * A, k["pas"], generator=gen) for _ in range(k["T"])]
    return [orc.device_noise(k["philox_seed"], 0, k["n"], t, k["pas"], L) for t in range(k["T_dev"] if T is None else T)]


def replay_reference(name, rng_mode, swap_every, energy, c, lib, noise=None, keep_probs=False, T=None):
    k = REPLAY_CASES[name]
    noise = replay_noise(name, rng_mode, c["L"], T) if noise is None else noise
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    ref = tempered_run(energy, np.tile(c["wt"].astype(np.int64), (k["n"], 1)), c["wt"], lambda t: noise[t], len(noise), lo, hi,
                       k["pas"], k["nmut"], REPLAY_BETAS, swap_every, seed=k["philox_seed"], allowed=lib, trace=True,
                       keep_probs=keep_probs)
    return noise, ref

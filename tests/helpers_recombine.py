"""TEST INFRASTRUCTURE for recombination (include/ppde_hip.h, ppde_chains_set_recombination): the rule restated on the host.

partners / cut / open_list / cross restate the pairing, the Philox draw, the open list and the children; `event` applies them to a
population; `outcomes` is the decision in fp64 on recorded values; `pair_matrix` is the exact Markov matrix of one event of a pair
over the joint states (x_a, x_b) of an enumerated case (helpers_reversible.exact_reversible_kernel's state space), with the cut
probabilities taken from the exact mulhi counts; `apply_event` / `joint_law_recombined` carry a joint law of a deme of D slots through
iterations and events. `fault` plants a wrong rule (the power of the law tests)."""
import numpy as np

import ppde_oracle as orc

CROSS_STREAM = 0x40000002
FAULTS = ("ratio_a", "write_a", "cap_one", "round0")


def partners(s, D, fault=None):
    """int [D]: the slot each slot of a deme is paired with at event s (circle method)."""
    m = D - 1
    r = 0 if fault == "round0" else s % m
    out = np.empty(D, np.int64)
    out[m], out[r] = r, m
    for i in range(m):
        if i != r:
            out[i] = (2 * r - i) % m
    return out


def open_list(L, min_pos, max_pos, words=None):
    """The open residues: those of [min_pos, max_pos] whose library word is not 0 (all of them without a library)."""
    l = np.arange(min_pos, max_pos + 1)
    return l if words is None else l[np.asarray(words)[l] != 0]


def draw(seed, a, it, chain_offset=0):
    """Philox words [len(a), 4] of the pairs whose lower chains have the GLOBAL indices `a`, at iteration `it`."""
    a = np.asarray(a, dtype=np.uint64).reshape(-1)
    k = np.array([seed & 0xffffffff, ((seed >> 32) ^ (int(chain_offset) >> 32)) & 0xffffffff], dtype=np.uint32)
    ctr = np.zeros((a.size, 4), dtype=np.uint32)
    ctr[:, 0] = (a & 0xffffffff).astype(np.uint32); ctr[:, 1] = it; ctr[:, 2] = CROSS_STREAM
    return orc.philox4x32(ctr, k)


def cut(seed, a, it, S_o):
    """(lo, hi, u) of those pairs: indices into the open list and the uniform of the decision (fp32, 24 bits)."""
    w = draw(seed, a, it).astype(np.uint64)
    i1, i2 = (w[:, 0] * np.uint64(S_o)) >> np.uint64(32), (w[:, 1] * np.uint64(S_o)) >> np.uint64(32)
    u = (w[:, 2] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.minimum(i1, i2).astype(np.int64), np.maximum(i1, i2).astype(np.int64), u


def cut_probabilities(S_o):
    """{(lo, hi): probability}, exact: mulhi32(x, S_o) = i for ceil((i + 1) 2^32 / S_o) - ceil(i 2^32 / S_o) of the 2^32 words."""
    edge = [-((-(i << 32)) // S_o) for i in range(S_o + 1)]
    p = np.array([edge[i + 1] - edge[i] for i in range(S_o)], dtype=np.float64) / 2.0 ** 32
    return {(lo, hi): float(p[lo] * p[hi] * (1 if lo == hi else 2)) for lo in range(S_o) for hi in range(lo, S_o)}


def cross(xa, xb, sites):
    """The two children: xa with xb's letters at `sites`, and xb with xa's."""
    ca, cb = np.array(xa, copy=True), np.array(xb, copy=True)
    ca[..., sites], cb[..., sites] = np.asarray(xb)[..., sites], np.asarray(xa)[..., sites]
    return ca, cb


def event(X, wt, sites, s, it, D, seed, chain_offset=0, fault=None):
    """What event s behind iteration `it` proposes for the population X [n, L] of an object that starts at `chain_offset`:
    dict of partner (local), lo, hi, differ, child_dist [n], children [n, L] (each slot's own child), u [n]."""
    X = np.asarray(X)
    n = X.shape[0]
    partner = (np.arange(n) // D) * D + np.tile(partners(s, D, fault), n // D)
    a = np.minimum(np.arange(n), partner)
    lo, hi, u = cut(seed, chain_offset + a, it, len(sites))
    children = X.copy()
    differ = np.zeros(n, np.int64)
    for i in range(n):
        seg = np.asarray(sites)[lo[i]:hi[i] + 1]
        children[i, seg] = X[partner[i], seg]
        differ[i] = int((X[i, seg] != X[partner[i], seg]).sum())
    child_dist = (children != np.asarray(wt)[None]).sum(1)
    return dict(partner=partner, lo=lo, hi=hi, differ=differ, child_dist=child_dist, children=children, u=u)


def recombined_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length, nmut_threshold, every, D, seed, allowed,
                   chain_offset=0, fault=None, trace=False, keep_probs=False, forbidden=None, motif_fault=None):
    """The CPU iteration of reversible mode (helpers_reversible.reversible_iteration) on explicit noise with the events of the
    rule: dict of states [T + 1, n, L], energy_history / fitness_history [T + 1, n] (row it + 1 after the event), accepted
    [T, n] (the slots' own Metropolis results) and the event records partner, lo, hi, differ, child_dist, outcome, log_ratio,
    pre_energy, child_energy [events, n]. `trace`: also traces (the iterations' dicts; `keep_probs`: with their forward rows),
    post_accept (states, energies per iteration, in front of the event) and the running best by the accept phase's strict rule
    (best_idx, best_energy, best_fitness, best_step), as helpers_anneal.annealed_run keeps them.
    `forbidden` = (patterns, allow_native): the iteration runs through helpers_motifs' constrained iteration, a pair with a child
    that is not free takes outcome 4 (`outcome_of`), and the result gains vetoes int64 [n, M], which the children never enter
    (`motif_fault`: one of helpers_motifs' faults)."""
    import torch
    import helpers_motifs as hmot
    import helpers_reversible as hr
    from ppde_amd import library as dl
    thr = hr._threshold(nmut_threshold)
    cur = torch.as_tensor(np.asarray(idx0)).long()
    wt = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    n, L = cur.shape
    words = dl.as_words(allowed, L)
    sites = open_list(L, min_pos, max_pos, words)
    e0, f0 = energy.energy(cur)
    e_hist, f_hist, states, accs = [e0.numpy()], [f0.numpy()], [cur.numpy().copy()], []
    rec = {k: [] for k in ("partner", "lo", "hi", "differ", "child_dist", "outcome", "log_ratio", "pre_energy", "child_energy")}
    traces, post = [], []
    best_e, best_f, best_t, best_x = e0.numpy().copy(), f0.numpy().copy(), np.zeros(n, np.int64), cur.numpy().copy()

    def take_best(e_row, f_row, x_rows, t):
        better = e_row > best_e                                              # strict: the accept phase's rule
        best_e[better], best_f[better], best_t[better], best_x[better] = e_row[better], f_row[better], t, x_rows[better]

    iteration, con = hmot.iteration_of(forbidden, n, motif_fault)
    for it in range(num_steps):
        U, q, u = noise(it)
        out = iteration(energy, cur, wt, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=keep_probs)
        cur = out["idx"].clone()
        e, f = out["energy"].numpy().copy(), out["fitness"].numpy().copy()
        accs.append(out["accepted"].numpy())
        if trace:
            traces.append(out)
            post.append((cur.numpy().copy(), e.copy()))
            take_best(e, f, cur.numpy(), it + 1)
        if (it + 1) % every == 0:
            ev = event(cur.numpy(), wt.numpy(), sites, (it + 1) // every - 1, it, D, seed, chain_offset, fault)
            ce, cf = (t.numpy() for t in energy.energy(torch.as_tensor(ev["children"]).long()))
            pa = ev["partner"]
            a, b = np.minimum(np.arange(n), pa), np.maximum(np.arange(n), pa)
            d = ((ce[a] - e[a]) + (ce[b] - e[b])).astype(np.float32)
            with np.errstate(over="ignore"):
                hit = np.exp(d) >= ev["u"]
            finite = np.isfinite(ce) & np.isfinite(ce[pa])
            capped = (ev["child_dist"] >= thr) | (ev["child_dist"][pa] >= thr)
            free = None if con is None else con.children_free(ev["children"], wt.numpy(), pa)
            outcome = outcome_of(finite, capped, free, hit).astype(np.uint8)
            for k, v in (("partner", pa), ("lo", ev["lo"]), ("hi", ev["hi"]), ("differ", ev["differ"]), ("child_dist", ev["child_dist"]),
                         ("outcome", outcome), ("log_ratio", d), ("pre_energy", e.copy()), ("child_energy", ce)):
                rec[k].append(np.asarray(v))
            acc = outcome == 1
            cur = torch.as_tensor(np.where(acc[:, None], ev["children"], cur.numpy())).long()
            e, f = np.where(acc, ce, e), np.where(acc, cf, f)
            if trace:
                take_best(e, f, cur.numpy(), it + 1)
        e_hist.append(e)
        f_hist.append(f)
        states.append(cur.numpy().copy())
    res = dict(states=np.stack(states), energy_history=np.stack(e_hist), fitness_history=np.stack(f_hist),
               accepted=np.stack(accs) if accs else np.zeros((0, n), bool))
    res.update({k: np.stack(v) if v else np.zeros((0, n)) for k, v in rec.items()})
    if trace:
        res.update(traces=traces, post_accept=post, best_idx=best_x, best_energy=best_e, best_fitness=best_f, best_step=best_t)
    if con is not None:
        res.update(vetoes=con.vetoes, veto_log=con.log)
    return res


def outcome_of(finite, capped, pair_free, hit):
    """The outcome of every slot's pair: 3 a non-finite child energy, 2 a child at or over the cap, 4 a child that is not free
    (`pair_free` bool [n], None without forbidden patterns) -- checked behind 3 and 2 and in front of u --, then 1 / 0 by u."""
    out = np.where(hit, 1, 0)
    if pair_free is not None:
        out = np.where(pair_free, out, 4)
    return np.where(~finite, 3, np.where(capped, 2, out))


def outcomes(log_ratio, u, child_dist, partner, child_energy, nmut, pair_free=None):
    """The decision in fp64 on recorded values: (outcome [n], margin [n] = |exp(d) - u| / max(exp(d), u) where u decided).
    `pair_free` bool [n]: forbidden patterns are set and both children of the slot's pair are free (outcome 4 where not)."""
    d = np.asarray(log_ratio, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ed = np.exp(d)
    finite = np.isfinite(child_energy) & np.isfinite(np.asarray(child_energy)[partner])
    capped = (nmut > 0) & ((child_dist >= nmut) | (np.asarray(child_dist)[partner] >= nmut)) if nmut > 0 else np.zeros(d.size, bool)
    out = outcome_of(finite, capped, pair_free, ed >= u)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.where(finite & ~capped, np.abs(ed - u) / np.maximum(ed, u), np.inf)
    return out, margin


def pair_matrix(states, positions, E, inside, fault=None):
    """X float64 [S^2, S^2] over joint states (x_a, x_b) (index x_a S + x_b): one event of a pair. `states` int [S, L] (every
    combination of the open residues' letters), `positions` the open list, E the oracle's fp32 energies [S], inside bool [S] = the
    states under the mutation cap (a child outside is rejected). Acceptance min(1, exp(d)), d in fp32 in the rule's order."""
    st = np.asarray(states)
    S = st.shape[0]
    E32 = np.asarray(E, dtype=np.float32)
    key = {tuple(int(v) for v in row[positions]): i for i, row in enumerate(st)}
    xa, xb = (g.reshape(-1) for g in np.meshgrid(np.arange(S), np.arange(S), indexing="ij"))
    J = S * S
    X = np.zeros((J, J))
    for (lo, hi), p in cut_probabilities(len(positions)).items():
        seg = np.asarray(positions)[lo:hi + 1]
        ca_rows, cb_rows = cross(st[xa], st[xb], seg)
        ca = np.array([key[tuple(int(v) for v in r[positions])] for r in ca_rows])
        cb = np.array([key[tuple(int(v) for v in r[positions])] for r in cb_rows])
        if fault == "ratio_a":
            d = E32[ca] - E32[xa]
        else:
            d = (E32[ca] - E32[xa]) + (E32[cb] - E32[xb])
        with np.errstate(over="ignore"):
            acc = np.minimum(1.0, np.exp(d.astype(np.float32).astype(np.float64)))
        ok = inside[ca] if fault == "cap_one" else inside[ca] & inside[cb]
        acc = np.where(ok, acc, 0.0)
        to = ca * S + (xb if fault == "write_a" else cb)
        np.add.at(X, (np.arange(J), to), p * acc)
        np.add.at(X, (np.arange(J), np.arange(J)), p * (1.0 - acc))
    return X


def apply_kernel(v, K, D):
    """The joint law v [S^D] (slot 0 slowest) after every slot took one step of K."""
    S = K.shape[0]
    t = v.reshape((S,) * D)
    for ax in range(D):
        t = np.moveaxis(np.tensordot(t, K, axes=([ax], [0])), -1, ax)
    return t.reshape(-1)


def apply_event(v, X, s, D, S, fault=None):
    """The joint law after event s: the pair matrix on every pair of the matching (`fault` 'round0': the pairing stuck at round 0)."""
    t = v.reshape((S,) * D)
    pr = partners(s, D, fault)
    for a in range(D):
        b = int(pr[a])
        if a > b:
            continue
        t = np.moveaxis(t, (a, b), (D - 2, D - 1))
        shape = t.shape
        t = (t.reshape(-1, S * S) @ X).reshape(shape)
        t = np.moveaxis(t, (D - 2, D - 1), (a, b))
    return t.reshape(-1)


def joint_law_recombined(T, K, X, every, D, start, fault=None):
    """The law of a deme's joint state (slot 0 slowest) after T iterations from the joint index `start`: K on every slot per
    iteration, the event's matrix behind iteration it when (it + 1) % every == 0."""
    S = K.shape[0]
    v = np.zeros(S ** D)
    v[start] = 1.0
    for it in range(T):
        v = apply_kernel(v, K, D)
        if (it + 1) % every == 0:
            v = apply_event(v, X, (it + 1) // every - 1, D, S, fault)
    return v


def case_c():
    """Case C of the law tests (D = 4): L = 8, Potts window 1..6, three open residues with two letters each: 8 states."""
    import helpers_tempering as ht
    c = ht.one_site_case(8, 6, 1, 2, letters=2, seed=43)
    rng = np.random.default_rng(43)
    for site in (4, 5):
        other = int((int(c["wt"][site]) + 1 + rng.integers(0, 19)) % 20)
        c["allowed"][site] = (1 << other) | (1 << int(c["wt"][site]))
    return c


LAW_T = (1, 2, 3, 8)
LAW_EVERY = (1, 3)
# joint start states from which the GPU law tests (2^16 pairs of case A, 2^15 demes of 4 of case C) can see every planted fault
# that applies (tests/test_recombine_cpu.py: test_the_law_tests_can_see_every_fault)
POWER_START_A = {0: (17, 3), 2: (12, 1)}     # by the mutation cap nmut of the run
POWER_START_C = (1, 2, 4, 7)

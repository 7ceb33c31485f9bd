"""The reference of forbidden patterns (ppde_chains_set_forbidden_patterns; tests/test_motifs_cpu.py, tests/test_motifs_gpu.py).

The rule itself is ppde_amd/motifs.py's `find`; here are a three-line brute force to hold it against, the CPU iteration of the
mode -- helpers_reversible's reversible iteration with the veto in the decision --, the exact constrained kernel, the law case's
patterns and the planted faults.

The exact kernel: helpers_reversible.exact_reversible_kernel enumerates every path of the unconstrained iteration. The constrained
iteration proposes along the same rows (only y is checked, never a path's intermediate states), scores with the same ratio and
rejects a y that is not free. So its matrix is the unconstrained one with `inside &= free`: the rows of free states only, the
flows into states that are not free returned to the diagonal. `constrain_kernel` does exactly that to the enumerated matrix."""
import numpy as np
import torch

import helpers_reversible as hr
from ppde_amd import motifs

A = 20
FAULTS = ("last_start_skipped", "frozen_not_context", "native_per_pattern", "veto_through_u", "one_child_only")


def brute_find(idx, pt, active):
    """first (pattern, position) by the definition: loops over patterns, starts and elements; active bool [M, L]."""
    out = []
    for x in np.asarray(idx):
        hits = [(m, p) for m in range(len(pt)) for p in range(len(x) - int(pt.lengths[m]) + 1) if active[m, p]
                and all((int(pt.elements[m, j]) >> int(x[p + j])) & 1 for j in range(int(pt.lengths[m])))]
        out.append(min(hits) if hits else (-1, -1))
    return np.array(out, np.int32).reshape(-1, 2).T


def faulty_active(pt, L, wt, allow_native, fault, allowed=None):
    """active bool [M, L] as a planted fault would form it (None: the rule)."""
    act = motifs.active_mask(pt, L, wt, allow_native)
    if fault == "last_start_skipped":
        for m in range(len(pt)):
            act[m, L - int(pt.lengths[m])] = False
    elif fault == "frozen_not_context":                      # windows over open residues only
        is_open = np.asarray(allowed) != 0
        for m in range(len(pt)):
            for p in range(L - int(pt.lengths[m]) + 1):
                act[m, p] &= bool(is_open[p:p + int(pt.lengths[m])].all())
    elif fault == "native_per_pattern" and allow_native:     # a pattern the wild type matches anywhere is exempt everywhere
        native = motifs.matches(np.asarray(wt).reshape(1, -1), pt)[0].any(axis=1)
        act[native] = False
    return act


def find_with(idx, pt, act):
    x = np.asarray(idx)
    hit = motifs.matches(x, pt) & act[None]
    any_m = hit.any(axis=2)
    fp = np.where(any_m.any(axis=1), any_m.argmax(axis=1), -1).astype(np.int32)
    pos = hit[np.arange(x.shape[0]), np.maximum(fp, 0)].argmax(axis=1)
    return fp, np.where(fp >= 0, pos, -1).astype(np.int32)


def constrained_iteration(energy, idx_cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, pt, allow_native=True, fault=None,
                          keep_probs=False, stale=None):
    """One iteration of the mode for all chains: hr.reversible_iteration's proposal, ratio and refusals, and the decision
    acc = exp(log_acc) >= u and not refused and y free. A vetoed proposal records what a cap rejection records: accept bit 0,
    the current state, energy and fitness; log_acc stays the computed value. Extra keys: veto bool [n], first_pattern int32 [n]
    (the pattern the counter counts), decided bool [n] (the vetoed proposals that u and the refusals would have let through).
    `fault`: one of FAULTS or RUN_FAULTS; `stale`: the veto of the iteration before ('veto_stale' decides by it)."""
    out = hr.reversible_iteration(energy, idx_cur, idx_cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=keep_probs)
    n = idx_cur.shape[0]
    y = out["proposal"].numpy()
    if fault in ("last_start_skipped", "frozen_not_context", "native_per_pattern"):
        act = faulty_active(pt, y.shape[1], np.asarray(wt_idx), allow_native, fault, _words(allowed, y.shape[1]))
        fp, _ = find_with(y, pt, act)
    else:
        act = motifs.active_mask(pt, y.shape[1], np.asarray(wt_idx), allow_native)
        fp, _ = motifs.find(y, pt, np.asarray(wt_idx), allow_native)
    veto = torch.as_tensor(fp >= 0)
    passed = (torch.exp(out["log_acc"]) >= u) & ~out["refused"]
    if fault == "veto_through_u":                            # -inf in the ratio instead of an explicit rejection: u = 0 accepts
        acc = (torch.exp(torch.where(veto, torch.tensor(-np.inf), out["log_acc"])) >= u) & ~out["refused"]
    elif fault == "veto_ignored":
        acc = passed
    elif fault == "veto_stale":                              # the byte the accept reads is the one the iteration before wrote
        acc = passed & ~(torch.zeros(n, dtype=torch.bool) if stale is None else stale)
    else:
        acc = passed & ~veto
    if fault == "highest_pattern_counted":
        any_m = (motifs.matches(y, pt) & act[None]).any(axis=2)
        fp = np.where(fp >= 0, any_m.shape[1] - 1 - any_m[:, ::-1].argmax(axis=1), -1).astype(np.int32)
    if fault == "counted_only_when_it_decided":
        fp = np.where(passed.numpy(), fp, -1).astype(np.int32)
    out.update(idx=torch.where(acc.reshape(n, 1), out["proposal"], idx_cur), energy=torch.where(acc, out["e_y"], out["e_x"]),
               fitness=torch.where(acc, out["fit_y"], out["fit_x"]), accepted=acc, veto=veto, first_pattern=fp, decided=veto & passed)
    return out


def _words(allowed, L):
    from ppde_amd import library as dl
    return dl.as_words(dl.full_library(L) if allowed is None else allowed, L)


# faults of a whole run, next to FAULTS: the accept phase deaf to the byte, or reading the byte of the iteration before (the veto
# enqueued behind the accept), recombination's children in the counters, a counter that counts only the vetoes that changed the
# outcome, the highest matching pattern in the counter cell
RUN_FAULTS = ("veto_ignored", "veto_stale", "children_counted", "counted_only_when_it_decided", "highest_pattern_counted")


class Constraint:
    """The mode as every reversible dynamics runs it, stated once: `iteration` is constrained_iteration on the energy object the
    mode's helper built (the beta-scaled one under tempering and annealing) and counts the counters as the header says -- the lowest
    matching active pattern, whether or not the proposal would otherwise have been accepted --; `children_free` is the check of a
    recombination event, whose children are not counted. forbidden = (patterns, allow_native)."""

    def __init__(self, forbidden, n, fault=None):
        self.pt, self.allow_native, self.fault = motifs.parse(forbidden[0]), bool(forbidden[1]), fault
        self.vetoes = np.zeros((n, len(self.pt)), np.int64)
        self.stale = None
        self.log = []                                        # per iteration (veto, first_pattern, decided)

    def iteration(self, energy, idx_cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, keep_probs=False):
        out = constrained_iteration(energy, idx_cur, wt_idx, U, q, u, min_pos, max_pos, thr, allowed, self.pt, self.allow_native,
                                    self.fault, keep_probs, self.stale)
        hit = np.flatnonzero(out["first_pattern"] >= 0)
        np.add.at(self.vetoes, (hit, out["first_pattern"][hit]), 1)
        self.stale = out["veto"]
        self.log.append((out["veto"].numpy().copy(), out["first_pattern"].copy(), out["decided"].numpy().copy()))
        return out

    def children_free(self, children, wt_idx, partner):
        """bool [n]: BOTH children of the slot's pair are free (an event's outcome 4 where not)."""
        fp, _ = motifs.find(np.asarray(children), self.pt, np.asarray(wt_idx), self.allow_native)
        if self.fault == "children_counted":
            hit = np.flatnonzero(fp >= 0)
            np.add.at(self.vetoes, (hit, fp[hit]), 1)
        free = fp < 0
        if self.fault == "one_child_only":                   # the lower slot's child alone
            return free[np.minimum(np.arange(free.size), np.asarray(partner))]
        return free & free[np.asarray(partner)]


def iteration_of(forbidden, n, fault=None):
    """(iteration, constraint) a mode helper runs: hr.reversible_iteration and None without patterns."""
    if forbidden is None:
        return (lambda energy, cur, wt, U, q, u, lo, hi, thr, allowed, keep_probs=False:
                hr.reversible_iteration(energy, cur, cur, wt, U, q, u, lo, hi, thr, allowed, keep_probs=keep_probs)), None
    c = Constraint(forbidden, n, fault)
    return c.iteration, c


def constrained_run(energy, idx0, wt_idx, noise, num_steps, min_pos, max_pos, pas_length, nmut_threshold, allowed, pt,
                    allow_native=True, fault=None, keep_probs=False):
    """hr.reversible_run with the mode on: the same dict (traces always), plus vetoes int64 [n, M]."""
    thr = hr._threshold(nmut_threshold)
    idx0 = torch.as_tensor(np.asarray(idx0)).long()
    wt = torch.as_tensor(np.asarray(wt_idx)).long().reshape(-1)
    n, L = idx0.shape
    if allowed is None:
        from ppde_amd import library as dl
        allowed = dl.full_library(L)
    e0, f0 = energy.energy(idx0)
    e_hist, f_hist, states, accs, traces = [e0], [f0], [idx0.clone()], [], []
    con = Constraint((pt, allow_native), n, fault)
    cur = idx0.clone()
    for it in range(num_steps):
        U, q, u = noise(it)
        out = con.iteration(energy, cur, wt, U, q, u, min_pos, max_pos, thr, allowed, keep_probs)
        cur = out["idx"].clone()
        e_hist.append(out["energy"]); f_hist.append(out["fitness"]); accs.append(out["accepted"]); traces.append(out)
        states.append(cur.clone())
    e_hist, f_hist, states = torch.stack(e_hist, 0), torch.stack(f_hist, 0), torch.stack(states, 0)
    best_e, best_t = torch.max(e_hist, 0)
    ar = torch.arange(n)
    return dict(best_idx=states[best_t, ar], best_energy=best_e, best_fitness=f_hist[best_t, ar], energy_history=e_hist,
                fitness_history=f_hist, states=states, accepted=torch.stack(accs, 0), final_idx=cur, traces=traces, vetoes=con.vetoes, veto_log=con.log)


def constrain_kernel(K, inside, free):
    """The constrained kernel from the enumerated unconstrained one (`inside &= free`, see the module's text): (K', inside')."""
    ins = np.asarray(inside) & np.asarray(free)
    Kc = np.array(K, dtype=np.float64)
    Kc[:, ~ins] = 0.0
    Kc[~ins, :] = 0.0
    for x in np.flatnonzero(ins):
        Kc[x, x] = 0.0
        Kc[x, x] = 1.0 - Kc[x].sum()
    return Kc, ins


def law_patterns(c):
    """The law case's patterns on helpers_reversible.cap_case(): n2 / n3 = the non-wild-type letters of residue 2 / 3, increasing;
    P0 = [n2[0:3]][n3[0:4]] at the two open residues, P1 = [wt[1]][n2[3:5]] with the frozen residue 1 as context, P2 =
    [n3[4:6]][wt[4]] with the frozen residue 4."""
    wt = c["wt"]
    n2 = [k for k in range(A) if (int(c["allowed"][2]) >> k) & 1 and k != int(wt[2])]
    n3 = [k for k in range(A) if (int(c["allowed"][3]) >> k) & 1 and k != int(wt[3])]
    bits = lambda ks: sum(1 << int(k) for k in ks)
    el = np.zeros((3, 8), np.uint32)
    el[0, :2] = [bits(n2[0:3]), bits(n3[0:4])]
    el[1, :2] = [bits([wt[1]]), bits(n2[3:5])]
    el[2, :2] = [bits(n3[4:6]), bits([wt[4]])]
    return motifs.Patterns(el, [2, 2, 2])


def random_patterns(rng, M=32, density=0.35, max_len=8):
    """M patterns of lengths 1..max_len in turn, every element a random non-empty set."""
    el = np.zeros((M, 8), np.uint32)
    ln = np.array([1 + m % max_len for m in range(M)], np.int32)
    for m in range(M):
        for j in range(int(ln[m])):
            w = 0
            while w == 0:
                w = int(sum(1 << k for k in range(A) if rng.random() < density))
            el[m, j] = w
    return motifs.Patterns(el, ln)


def plant(row, pt, m, p, rng):
    """`row` with a match of pattern m planted at start p."""
    r = np.array(row)
    for j in range(int(pt.lengths[m])):
        letters = [k for k in range(A) if (int(pt.elements[m, j]) >> k) & 1]
        r[p + j] = letters[int(rng.integers(len(letters)))]
    return r


# ------------------------------------------------------------------------------------------------ the replay cases
# helpers_reversible's replay cases (TOY24, Potts + CNN, the seeded library, chains from the wild type, the same seeds) under these
# patterns: a letter class anywhere, a pair and a triple with a wildcard. They were picked on the REFERENCE alone:
# tests/test_motifs_cpu.py asserts that they veto at least a tenth of its proposals and that none of its decisions or races comes
# closer to a tie than tests/test_reversible_cpu.py's margins.
REPLAY_PATTERNS = "[LRY], x[FHV], [GT]x[FHV]"
REPLAY_NAMES = ("pas2", "pas2_cap3", "pas3")


def replay_reference(name, rng_mode, energy, c, lib, noise=None, keep_probs=False):
    k = hr.REPLAY_CASES[name]
    noise = hr.replay_noise(name, rng_mode, c["L"]) if noise is None else noise
    lo, hi = c["i0"], c["i0"] + c["Lp"] - 1
    pt = motifs.parse(REPLAY_PATTERNS)
    ref = constrained_run(energy, np.tile(c["wt"].astype(np.int64), (k["n"], 1)), c["wt"], lambda t: noise[t], len(noise), lo, hi, k["pas"],
                          k["nmut"], lib, pt, keep_probs=keep_probs)
    return noise, ref, pt


def veto_share(ref):
    return float(ref["vetoes"].sum()) / (ref["accepted"].shape[0] * ref["accepted"].shape[1])

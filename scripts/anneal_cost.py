#!/usr/bin/env python3
"""What population annealing costs a reversible run: PABP-shaped Potts + CNN product of experts, 128 chains in one
deme of 128, device RNG, hipGraph replay, gradient reuse, no trace, a library of all letters over the Potts window -- against a
one-rung tempering run of the same shape, which has the same unfused flow (propose, experts, accept, one population kernel) and
whose code this mode does not touch.

  tempering1   set_tempering((1.0,), swap_every 1): k_propose_temp, k_accept_temp, k_swap
  idle         set_annealing((1, 1), every 1): one stage behind iteration 0 (in the warm-up), then both selection kernels return on
               their first branch in every timed iteration: the price of the two early-exit launches
  sparse       set_annealing(linspace(0.25, 1, 41), every 50): the way the mode is meant to be run
  events       set_annealing(4096 stages of 0.25 -> 1, every 1): a selection behind EVERY timed iteration: the event's own time
               (a schedule has at most 4096 stages, so this variant's rounds are shorter: warm-up + rounds x steps <= 4096)
  fixed10, fixed100        set_annealing(0.25 -> 1 in as many stages as events fit, every 10 / 100)
  adaptive, adaptive10, adaptive100   set_annealing_adaptive(0.25, 1, --ess, every 1 / 10 / 100, min_step 2^-20): DESIGN.md §4.2k, the
               same number of events as events / fixed10 / fixed100. An event of a deme that has not arrived costs one fp64
               workgroup reduction (the whole remainder passes) or 49 (the bisection); which of the two each timed event was is
               read back from the recorded beta pairs and reported next to the time
  adaptive_search          set_annealing_adaptive(0.25, 64, 0.999999, every 1, min_step 64 x 2^-20): a target and an end chosen so that
               the deme never arrives and every timed event runs all 49 reductions -- against `events`, which has an event behind
               every iteration too, the difference is the search itself

  python scripts/anneal_cost.py [--steps 2000] [--rounds 5] [--out profiles/anneal_step_cost.md]

One process; the variants are timed in turn, `--rounds` times over (alternating, so drift of the machine hits all alike), each
timing a host clock around `--steps` iterations that end in a device synchronise, after a warm-up of 200. Reported: the median
and the range over the rounds, in microseconds per iteration."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BOUNDARY_US = 1.45          # a dependent boundary between trivial kernels on the MI355X (MI355X_MICROARCH.md's price table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--ess", type=float, default=0.999, help="ESS target of the adaptive variants (close to 1: many small steps, so "
                                                             "that most timed events run the bisection)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "anneal_step_cost.md"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from ppde_amd import library, synthetic
    from ppde_amd.encoding import seqs_to_idx
    from ppde_amd.energy import HipModel
    from ppde_amd.sampler import Chains
    _, seq, (i0, Lp) = synthetic.PROTEINS["PABP_YEAST_Fields2013"]
    wt = seqs_to_idx([seq])[0]
    L, n = len(wt), a.chains
    J, h = synthetic.make_potts(Lp, seed=1234)
    m = HipModel(wt, "cuda:0")
    m.set_potts(J, h, i0)
    m.set_cnn([synthetic.make_cnn_state(L, s) for s in range(3)])
    m.set_lamda(5.0)
    T = a.warmup + a.rounds * a.steps
    variants = {
        "tempering1": lambda ch: ch.set_tempering((1.0,), 1),
        "idle": lambda ch: ch.set_annealing((1.0, 1.0), 1, n),
        "sparse": lambda ch: ch.set_annealing(np.linspace(0.25, 1.0, 41), 50, n),
        "events": lambda ch: ch.set_annealing(np.linspace(0.25, 1.0, 4097), 1, n),
        "adaptive": lambda ch: ch.set_annealing_adaptive(0.25, 1.0, a.ess, 1, n, 4096, 2.0 ** -20),
        "adaptive_search": lambda ch: ch.set_annealing_adaptive(0.25, 64.0, 0.999999, 1, n, 4096, 64 * 2.0 ** -20),
    }
    every_of = {k: 1 for k in variants}
    every_of["sparse"] = 50
    for k in (10, 100):
        stages = min(4096, T // k)
        variants[f"fixed{k}"] = lambda ch, k=k, stages=stages: ch.set_annealing(np.linspace(0.25, 1.0, stages + 1), k, n)
        variants[f"adaptive{k}"] = lambda ch, k=k: ch.set_annealing_adaptive(0.25, 1.0, a.ess, k, n, 4096, 2.0 ** -20)
        every_of[f"fixed{k}"] = every_of[f"adaptive{k}"] = k
    chains = {}
    for name, setup in variants.items():
        ch = Chains(m, n, T, 2, 0, False, 0, L - 1, 3, 1, reuse_grad=True, random_chain=-1, seed=1, use_graph=True)
        ch.set_library(library.fold_range(library.full_library(L), i0, i0 + Lp - 1))
        ch.set_reversible(True)
        setup(ch)
        ch.init(torch.as_tensor(np.tile(wt, (n, 1))).cuda())
        ch.run(a.warmup)
        ch.sync()
        chains[name] = ch
    us = {k: [] for k in variants}
    steps_of = {k: a.steps for k in variants}
    steps_of["events"] = steps_of["adaptive"] = steps_of["adaptive_search"] = min(a.steps, (4096 - a.warmup) // a.rounds)   # every timed iteration of them has an event
    for _ in range(a.rounds):
        for name, ch in chains.items():
            t0 = time.perf_counter()
            ch.run(steps_of[name])
            ch.sync()
            us[name].append((time.perf_counter() - t0) / steps_of[name] * 1e6)
    notes = {}
    timed = {}                                                               # adaptive variants: (events, bisected, one reduction) in the timed iterations
    for name in variants:
        if name == "tempering1":
            continue
        st = chains[name].annealing_state()
        notes[name] = f"{st['events']} events, {int((st['parent'] != np.arange(n)[None]).sum())} slots replaced, smallest ESS {st['ess'].min():.1f}"
        if name.startswith("adaptive"):
            k, first = every_of[name], a.warmup // every_of[name]            # (events 0 .. first - 1 lie in the warm-up)
            last = min(st["events"], (a.warmup + a.rounds * steps_of[name]) // k)
            before, after = st["beta_before"][first:last, 0], st["beta_after"][first:last, 0]
            end = 64.0 if name == "adaptive_search" else 1.0
            timed[name] = (last - first, int((after < end).sum()), int(((before < end) & (after >= end)).sum()))
            notes[name] += (f"; timed: {timed[name][0]} events, {timed[name][1]} bisected (49 reductions), {timed[name][2]} arrivals (1 to 49), "
                            f"{timed[name][0] - timed[name][1] - timed[name][2]} after arrival (none)")
    notes["tempering1"] = "-"
    med = {k: float(np.median(v)) for k, v in us.items()}
    lines = ["# Cost of population annealing per iteration (scripts/anneal_cost.py)", "",
             f"PABP-shaped Potts + CNN product of experts (L = {L}, window {Lp}), {n} chains, one deme of {n}, device RNG, hipGraph replay, gradient",
             f"reuse, a library of all letters over the window. {a.rounds} rounds of {a.steps} iterations per variant, taken in turn in one process, a host",
             f"clock around iterations that end in a device synchronise (`events`: {steps_of['events']} per round, all of them with an event);",
             "microseconds per iteration, median (smallest .. largest round).", "",
             "| run | us / iteration | against tempering1 | events |", "|---|---|---|---|"]
    for name in variants:
        lines.append(f"| {name} | {med[name]:.2f} ({min(us[name]):.2f} .. {max(us[name]):.2f}) | {med[name] - med['tempering1']:+.2f} | {notes[name]} |")
    sparse_events = chains["sparse"].annealing_state()["events"]
    lines += ["",
              f"`tempering1` is a one-rung ladder with a swap event behind every iteration: propose, experts, accept and `k_swap`, unfused, the code of",
              "the parent commit (this mode does not touch it). `idle` has the same flow with `k_select_plan` and `k_select_copy` in `k_swap`'s place,",
              f"both returning on their first branch: it carries one launch more than `tempering1`, so the price table of MI355X_MICROARCH.md",
              f"(a dependent boundary between trivial kernels: {BOUNDARY_US} us; 1.7-1.9 us between real streaming kernels) predicts",
              f"{BOUNDARY_US:+.2f} us; measured {med['idle'] - med['tempering1']:+.2f} us. What the two early-exit launches cost in absolute terms is not",
              "separated here: every unfused flow of this library has a population kernel, so there is no run without one to subtract. An",
              "early-exit launch is not an empty kernel: before its first branch it loads the device iteration counter (one dependent scalar",
              "load from memory, as in `k_swap`), and `k_select_copy` is a grid of one workgroup per chain where `k_swap` has one workgroup;",
              "whether that accounts for the difference to the guide's figure has not been measured.",
              f"`events` pays a selection behind every iteration: the event's own time is {med['events'] - med['idle']:.2f} us (events - idle), the plan",
              "of one deme of 128 (one workgroup) and the copy launch (128 workgroups, the replaced ones copying a row).",
              f"`sparse` ({sparse_events} events in {a.warmup + a.rounds * a.steps} iterations) is the mode as it is meant to be run."]
    lines += ["", "## The adaptive form (DESIGN.md §4.2k)", "",
              f"`adaptive*` choose each step on the device (ESS target {a.ess:g}, 0.25 -> 1, min_step 2^-20) and are set against the fixed-schedule",
              "run with the same number of events at the same `every`. The difference is what the search costs; an event after the deme's",
              "arrival searches nothing, so the difference is also given per bisected event (difference x timed iterations / bisected events;",
              "`-` when no timed event bisected).", "",
              "| every | fixed us / iteration | adaptive us / iteration | difference per iteration | per event (x every) | per bisected event |",
              "|---|---|---|---|---|---|"]
    for k, fx, ad in ((1, "events", "adaptive"), (10, "fixed10", "adaptive10"), (100, "fixed100", "adaptive100")):
        d = med[ad] - med[fx]
        bis = timed[ad][1]
        per_bis = f"{d * a.rounds * steps_of[ad] / bis:.2f}" if bis else "-"
        lines.append(f"| {k} | {med[fx]:.2f} ({min(us[fx]):.2f} .. {max(us[fx]):.2f}) | {med[ad]:.2f} ({min(us[ad]):.2f} .. {max(us[ad]):.2f}) | "
                     f"{d:+.2f} | {d * k:+.2f} | {per_bis} |")
    d = med["adaptive_search"] - med["events"]
    ev, bis, _ = timed["adaptive_search"]
    lines += ["",
              f"`adaptive_search` (0.25 -> 64 at an ESS target of 0.999999: {bis} of its {ev} timed events ran the bisection, the deme at beta = "
              f"{float(chains['adaptive_search'].annealing_state()['beta'][0]):.4g} at the end) against `events`: {med['adaptive_search']:.2f} "
              f"({min(us['adaptive_search']):.2f} .. {max(us['adaptive_search']):.2f}) - {med['events']:.2f} = {d:+.2f} us per event for the search of "
              f"one deme of {n}, {d / 49:.3f} us per fp64 workgroup reduction (4 fp64 exp per thread, two DPP wave sums, one barrier)."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    for ch in chains.values():
        ch.close()
    m.close()


if __name__ == "__main__":
    main()

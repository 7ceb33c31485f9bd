#!/usr/bin/env python3
"""Random configurations of the chain modes (default, reversible, tempering, fixed and adaptive annealing, recombination; each with
and without a design library; the four observers on half of them) at random geometries, on the device RNG, against the modes' CPU
references fed the device's noise restated on the CPU (tests/helpers_fuzz_modes.py: draw, reference, compare). No chain is exempt:
only draws whose reference run takes no decision near a tie are kept. FZ_FORBID=1: every configuration also carries forbidden
patterns built on its own unconstrained reference (the reversible dynamics only), and the veto counters, the active words and
outcome 4 join the comparison.
Run on the GPU box: python tests/fuzz_modes.py [seed]; FZ_TRIALS trials (default 12), FZ_DYNAMICS a comma list that restricts the
dynamics. PPDE_GRAPH_LEN (read once per process by the library) lets the short runs replay graphs: the generator then draws runs
that do, and the script demands that every dynamics it ran replayed some steps. Prints one line per trial and `failures: N`; exits non-zero on a mismatch. An
exception from the library ends the script there."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import helpers_fuzz_modes as fz
from ppde_amd.energy import HipModel
from ppde_amd.sampler import Chains

TWIN_KEYS = ("energy_history", "fitness_history", "best_idx", "best_step", "random_traj")


def build(cfg, m, trace):
    """Chains of `cfg` with the mode setters called in the order the header demands, initialised."""
    ob, dyn = cfg["observers"], cfg["dynamics"]
    ch = Chains(m, cfg["n"], cfg["T"], cfg["pas"], cfg["nmut"], False, cfg["min_pos"], cfg["max_pos"], cfg["which"], 1, trace=trace,
                random_chain=0, seed=cfg["seed"], reuse_grad=cfg["reuse_grad"], use_graph=cfg["use_graph"],
                chain_offset=cfg["chain_offset"], n_streams=cfg["n_streams"])
    if cfg["library"] is not None:
        ch.set_library(cfg["library"])
    if dyn != "default":
        ch.set_reversible(True)
    if dyn == "tempering":
        ch.set_tempering(cfg["betas"], cfg["swap_every"])
    elif dyn == "anneal":
        ch.set_annealing(cfg["schedule"], cfg["every"], cfg["deme"])
    elif dyn == "adaptive":
        ch.set_annealing_adaptive(cfg["beta_start"], cfg["beta_end"], cfg["ess_target"], cfg["every"], cfg["deme"], cfg["max_stages"],
                                  cfg["min_step"])
    elif dyn == "recombine":
        ch.set_recombination(cfg["every"], cfg["deme"])
    if cfg.get("patterns") is not None:                                       # (between create and init, behind set_reversible)
        ch.set_forbidden(cfg["patterns"], cfg["allow_native"])
    if ob is not None:
        ch.set_recorder(ob["every"], ob["burn_in"], ob["rung"], True)
        ch.set_pair_counts(ob["sites"])
        ch.set_archive(ob["K"])
        ch.set_stats(True)
    ch.init(torch.as_tensor(cfg["start"]).cuda())
    return ch


def device_run(cfg, m):
    """The drawn run() cuts with a peek at each, then every mode's state, in helpers_fuzz_modes' layout."""
    dyn = cfg["dynamics"]
    ch = build(cfg, m, True)
    peeks = []
    for k in cfg["cuts"]:
        ch.run(k)
        peeks.append(ch.peek())
    ch.sync()
    run = dict(tr=ch.trace(), res=ch.collect(), peeks=peeks, temp=None, anneal=None, recomb=None, graph=ch.graph_stats())
    if dyn == "tempering":
        run["temp"] = dict(ch.tempering_state(), hist=ch.tempering_history())
    if dyn in ("anneal", "adaptive"):
        run["anneal"] = ch.annealing_state()
    if dyn == "recombine":
        run["recomb"] = ch.recombination_state()
    if cfg.get("patterns") is not None:
        run["forbid"] = ch.forbidden_state()
    if cfg["observers"] is not None:
        run.update(rec=ch.recorded(), pairs=ch.pair_counts(), archive=ch.archive(), stats=ch.stats())
    ch.close()
    return run


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    trials = int(os.environ.get("FZ_TRIALS", 12))
    pool = tuple(os.environ["FZ_DYNAMICS"].split(",")) if os.environ.get("FZ_DYNAMICS") else None
    graph_len = int(os.environ.get("PPDE_GRAPH_LEN", 0) or 0)
    forbid = os.environ.get("FZ_FORBID", "0") not in ("", "0")
    t0 = time.time()
    configs, discarded = fz.kept(seed, trials, pool, graph_len, forbid)
    print(f"{trials} configurations kept, {discarded} discarded near a tie{' or without a veto' if forbid else ''} ({time.time() - t0:.1f} s of CPU reference)", flush=True)
    bad, replayed = 0, {}
    for trial, (cfg, ref) in enumerate(configs):
        print(f"trial {trial}: {fz.describe(cfg)}", flush=True)
        J, h, cnn = fz.model_parts(cfg)
        m = HipModel(cfg["wt"], "cuda:0")
        m.set_potts(J, h, cfg["i0"])
        if cnn:
            m.set_cnn(cnn)
        m.set_lamda(cfg["lamda"])
        t1 = time.time()
        run = device_run(cfg, m)
        why = fz.compare(cfg, run, ref)
        want = fz.replayed_steps(cfg, graph_len)
        gs = run["graph"]
        if gs["replayed_steps"] != want or gs["eager_steps"] != cfg["T"] - want or gs["captures_in_run"]:
            why.append(f"graph replay: {gs} against {want} replayed steps of {cfg['T']}")
        replayed[cfg["dynamics"]] = replayed.get(cfg["dynamics"], 0) + gs["replayed_steps"]
        if cfg["dynamics"] == "default":
            # the same run without trace buffers takes the SPECIALISED chain kernels where the configuration has one (and the
            # general ones under PPDE_CHAIN_SPEC=0): histories and best states must equal the traced run's bit for bit
            twin = build(cfg, m, False)
            for k in cfg["cuts"]:
                twin.run(k)
            res2 = twin.collect()
            twin.close()
            if not all(np.array_equal(run["res"][k], res2[k]) for k in TWIN_KEYS):
                why.append("the run without trace buffers differs from the traced run")
        bad += bool(why)
        de = np.abs(run["res"]["energy_history"] - ref["run"]["res"]["energy_history"]).max()
        vetoed = f"vetoes {int(run['forbid']['vetoes'].sum())}, " if forbid else ""
        print(f"   -> {'ok' if not why else 'FAIL: ' + '; '.join(why[:8])} (max |dE| {de:.1e}, {vetoed}accepted {run['tr']['accepted'].mean():.2f}, "
              f"replayed {gs['replayed_steps']} of {cfg['T']}, device {time.time() - t1:.2f} s)", flush=True)
        m.close()
    print("replayed steps per dynamics:", replayed)
    if graph_len:                                                             # the knob must have made the short runs replay
        dry = [d for d, k in replayed.items() if k == 0]
        if dry:
            print(f"FAIL: PPDE_GRAPH_LEN={graph_len} and no trial of {dry} replayed a step")
            bad += 1
    print("failures:", bad)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

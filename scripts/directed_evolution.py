#!/usr/bin/env python3
"""Directed evolution of a protein with the PPDE sampler on an MI355X.

Counterpart of the reference's scripts/directed_evolution.py (same flags, same outputs under
results_path/protein/<sampler>_<signature>_<seed>_<timestamp>/: population.npy [n, L, 20] f32,
pred_fitness_scores.npy, oracle_fitness_scores.npy, potts_scores.npy, energy_scores.npy,
energy_history.npy [T+1, n], fitness_history.npy [T+1, n], config.txt). Only the pieces on the PPDE hot path
exist here: `--sampler PPDE` with `--unsupervised_expert potts | transformer | transformer-S | transformer-M |
transformer-L | potts+transformer` (the ESM-2 checkpoint must be in <hub_dir>/checkpoints/) and `--energy_function supervised`; the baseline samplers and
the MSA-Transformer scoring are out of scope.

Extra flags: --ppde_rng {torch,philox}, --ppde_seed, --ppde_reuse_grad {0,1}, --ppde_shard (with torchrun), --ppde_full_grad,
--ppde_timing; design library (the letters the sampler may propose per residue): --ppde_sites, --ppde_exclude, --ppde_library;
--ppde_reversible (chains that sample exp(energy)/Z over the library); --ppde_betas, --ppde_swap_every (parallel tempering of such
a run: a ladder of inverse temperatures with replica exchange); --ppde_sample_every, --ppde_sample_burn_in, --ppde_sample_rung,
--ppde_sample_counts_only, --ppde_sample_pairs (thinned samples of the population and per-site letter counts, recorded on the device: samples.npy
[rows, slots, L] uint8, sample_energy.npy, sample_fitness.npy, sample_chain.npy [rows, slots], site_counts.npy [L, 20]). A run with
a ladder also writes rung_history.npy [T+1, n], swap_attempts.npy and swap_accepts.npy [n / R, R - 1]. --ppde_forbid,
--ppde_forbid_file, --ppde_forbid_strict (forbidden sequence patterns of a reversible run: motif_vetoes.npy [n, M] int64 and
motif_patterns.txt).
"""
import argparse
import datetime
import json
import os
import random
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
torch.set_printoptions(threshold=5000)

from ppde_amd import library as design_library  # noqa: E402
from ppde_amd.encoding import read_fasta, seqs_to_idx, seqs_to_onehot  # noqa: E402
from ppde_amd.energy import ProteinProductOfExperts, ProteinSupervised  # noqa: E402
from ppde_amd.nets import AugmentedLinearRegression, proteins_potts_score  # noqa: E402
from ppde_amd.sampler import PPDE_PAS  # noqa: E402


def get_sampler(args, library=None):
    if args.sampler == "PPDE":
        # (a copy: the namespace itself is what config.txt records, and a mask is no JSON)
        # (--ppde_stats_no_sites alone switches the statistics on, without their per-residue counts)
        stats = "no-sites" if getattr(args, "ppde_stats_no_sites", False) else bool(getattr(args, "ppde_stats", False))
        return PPDE_PAS(argparse.Namespace(**{**vars(args), "ppde_library": library, "ppde_stats": stats,
                                              "ppde_forbid": forbidden_patterns_from_flags(args)}))
    raise NotImplementedError(f"--sampler {args.sampler}: only PPDE is implemented on the MI355X path "
                              "(simulated_annealing / MALA-approx / CMAES / Random are the paper's baselines)")


def forbidden_patterns_from_flags(args):
    """--ppde_forbid / --ppde_forbid_file -> the list of pattern texts, or None. The file holds one pattern (or a comma-separated
    list) per line; '#' starts a comment."""
    items = []
    text, path = getattr(args, "ppde_forbid", None), getattr(args, "ppde_forbid_file", None)
    if text:
        items += [t.strip() for t in text.split(",")]
    if path is not None:
        with open(path) as f:
            for raw in f:
                line = raw.split("#", 1)[0].strip()
                if line:
                    items += [t.strip() for t in line.split(",")]
    return items or None


def design_library_from_flags(args, wt_idx, min_pos, max_pos):
    """--ppde_sites / --ppde_exclude / --ppde_library -> uint32 [L], or None when none of them is given. Positions are 0-based
    indices of the full sequence, the index space of the `min_pos max_pos` line the run prints."""
    sites, exclude, path = getattr(args, "ppde_sites", None), getattr(args, "ppde_exclude", "") or "", getattr(args, "ppde_library_file", None)
    if sites is None and not exclude and path is None:
        return None
    L = len(wt_idx)
    window = (int(min_pos), int(max_pos))
    if path is not None:            # replaces --ppde_sites; --ppde_exclude still applies on top of it
        lib = design_library.build_library(wt_idx, window, exclude=exclude, entries=design_library.parse_library_file(path, L))
    else:
        lib = design_library.build_library(wt_idx, window, exclude=exclude,
                                           sites=None if sites is None else design_library.parse_sites(sites, L))
    print(design_library.summary(lib), flush=True)
    return lib


def main(args):
    t_start = time.perf_counter()
    np.random.seed(args.seed)
    random.seed(args.seed)
    torch.manual_seed(args.seed)

    if args.run_signature == "":
        unique_token = "{}_{}_{}".format(args.sampler, args.seed, datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))
    else:
        unique_token = "{}_{}_{}_{}".format(args.sampler, args.run_signature, args.seed,
                                            datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S"))
    results_path = Path(args.results_path, args.protein, unique_token)
    if int(os.environ.get("RANK", 0)) == 0 or not args.ppde_shard:
        results_path.mkdir(parents=True, exist_ok=True)

    if args.ppde_shard and "RANK" in os.environ and not torch.distributed.is_initialized():
        # one process per GPU; PPDE_ONE_GPU=1 + PPDE_DIST_BACKEND=gloo rehearse several ranks on a single card
        local = 0 if os.environ.get("PPDE_ONE_GPU") else int(os.environ.get("LOCAL_RANK", 0))
        torch.cuda.set_device(local)
        args.device = f"cuda:{local}"
        torch.distributed.init_process_group(os.environ.get("PPDE_DIST_BACKEND", "nccl"))

    if args.energy_function == "product_of_experts":
        energy_func = ProteinProductOfExperts(args)
    elif args.energy_function == "supervised":
        energy_func = ProteinSupervised(args)
    else:
        raise ValueError(f"unknown --energy_function {args.energy_function}")
    energy_func = energy_func.to(args.device)

    dataset = os.path.join(args.protein_weights, args.protein)
    oracle = AugmentedLinearRegression(dataset, args.device)
    oracle.to(args.device)

    wtseqs = read_fasta(os.path.join(dataset, "wt.fasta"), return_ids=False)
    initial_population = torch.from_numpy(seqs_to_onehot(wtseqs)).float().to(args.device)
    initial_population = initial_population.repeat(args.n_chains, 1, 1)

    with torch.no_grad():
        print(f"WT protein energy: {energy_func.get_energy(initial_population)[0].mean():.3f}")

    library = design_library_from_flags(args, seqs_to_idx(wtseqs)[0], oracle.potts.index_list[0], oracle.potts.index_list[-1])
    sampler = get_sampler(args, library)
    t_loaded = time.perf_counter()
    best_samples, best_energy, best_fitness, energy_history, fitness_history, random_traj = \
        sampler.run(initial_population, args.n_iters, energy_func, oracle.potts.index_list[0],
                    oracle.potts.index_list[-1], oracle, args.log_every)

    t_sampled = time.perf_counter()
    best_oracle = oracle(best_samples).detach().cpu().numpy()
    potts_score = proteins_potts_score(best_samples, dataset).cpu().numpy()

    print(f"energy quantiles: {np.quantile(best_energy, [0.2, 0.4, 0.6, 0.8, 1.0])}")
    print(f"fitness quantiles: {np.quantile(best_fitness, [0.2, 0.4, 0.6, 0.8, 1.0])}")
    print(f"oracle quantiles: {np.quantile(best_oracle, [0.2, 0.4, 0.6, 0.8, 1.0])}")
    print(f"potts quantiles: {np.quantile(potts_score, [0.2, 0.4, 0.6, 0.8, 1.0])}")

    if not args.ppde_shard or not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
        with open(results_path / "config.txt", "w") as f:
            json.dump(args.__dict__, f, indent=2)
        np.save(results_path / "population.npy", best_samples.detach().cpu().numpy())
        np.save(results_path / "pred_fitness_scores.npy", best_fitness)
        np.save(results_path / "oracle_fitness_scores.npy", best_oracle)
        np.save(results_path / "potts_scores.npy", potts_score)
        np.save(results_path / "energy_scores.npy", best_energy)
        np.save(results_path / "energy_history.npy", energy_history)
        np.save(results_path / "fitness_history.npy", fitness_history)
        tempering = getattr(sampler, "tempering", None)
        if tempering is not None:
            for name in ("rung_history", "swap_attempts", "swap_accepts"):
                np.save(results_path / f"{name}.npy", tempering[name])
        annealing = getattr(sampler, "annealing", None)
        if annealing is not None:
            # (an adaptive run has no schedule: the path every deme chose takes the place of anneal_betas.npy)
            for name in ("parent", "pre_energy", "log_mean_w", "ess", "beta_path" if "beta_path" in annealing else "betas"):
                np.save(results_path / f"anneal_{name}.npy", annealing[name])
        recombination = getattr(sampler, "recombination", None)
        if recombination is not None:
            for name in ("partner", "cut", "differ", "outcome", "log_ratio", "pre_energy", "child_energy", "open_sites"):
                np.save(results_path / f"recomb_{name}.npy", recombination[name])
        samples = getattr(sampler, "samples", None)
        if samples is not None:
            np.save(results_path / "site_counts.npy", samples["site_counts"])
            if samples.get("pair_counts") is not None:
                np.save(results_path / "pair_counts.npy", samples["pair_counts"])
                np.save(results_path / "pair_sites.npy", samples["pair_sites"])
            if samples["idx"] is not None:
                np.save(results_path / "samples.npy", samples["idx"])
                np.save(results_path / "sample_energy.npy", samples["energy"])
                np.save(results_path / "sample_fitness.npy", samples["fitness"])
                np.save(results_path / "sample_chain.npy", samples["chain"])
        archive = getattr(sampler, "archive", None)
        if archive is not None:
            np.save(results_path / "archive.npy", archive["idx"])
            for name in ("energy", "fitness", "step", "count"):
                np.save(results_path / f"archive_{name}.npy", archive[name])
            cand = archive["candidates"]
            np.save(results_path / "candidates.npy", cand["idx"])
            for name, key in (("energy", "energy"), ("fitness", "fitness"), ("chain", "chain"), ("step", "step"), ("nchains", "n_chains")):
                np.save(results_path / f"candidates_{name}.npy", cand[key])
        forbidden = getattr(sampler, "forbidden", None)
        if forbidden is not None:
            np.save(results_path / "motif_vetoes.npy", forbidden["vetoes"])
            with open(results_path / "motif_patterns.txt", "w") as f:
                f.write("".join(t + "\n" for t in forbidden["text"]))
        stats = getattr(sampler, "stats", None)
        if stats is not None:
            for name in ("iters", "accepts", "moved", "jump_sum", "dist_sum", "wt_returns", "len_attempts", "len_accepts", "site_changes"):
                if stats[name] is not None:
                    np.save(results_path / f"stats_{name}.npy", stats[name])

    if not args.disable_MSA_transformer_scoring:
        print("MSA-Transformer scoring is not part of this build (needs the ESM-MSA-1b weights); skipped")
    print("done")
    if getattr(args, "ppde_timing", False):     # wall-clock split of this command (bench.py's also.paper_protocol reads this line)
        t_end = time.perf_counter()
        print("[ppde timing] " + json.dumps({"total_s": t_end - t_start, "load_s": t_loaded - t_start, "sampler_s": t_sampled - t_loaded,
                                             "score_and_save_s": t_end - t_sampled, **getattr(sampler, "timings", {})}), flush=True)
    if args.ppde_shard and torch.distributed.is_initialized():
        torch.distributed.barrier()
    return results_path


def build_parser():
    parser = argparse.ArgumentParser()
    g = parser.add_argument_group("general")
    g.add_argument("--protein_weights", type=str, default="weights")
    g.add_argument("--results_path", type=str, default="results/proteins")
    g.add_argument("--protein", type=str, default="PABP_YEAST_Fields2013",
                   help="PABP_YEAST_Fields2013, UBE4B_MOUSE_Klevit2013-nscor_log2_ratio, GFP_AEQVI_Sarkisyan2016")
    g.add_argument("--hub_dir", type=str, default=".")
    g.add_argument("--msa_path", type=str, default="data/proteins/PABP_YEAST.a2m")
    g.add_argument("--msa_size", type=int, default=500)
    g.add_argument("--seed", type=int, default=1234567)
    g.add_argument("--device", type=str, default="cuda")
    g.add_argument("--log_every", type=int, default=50)
    g.add_argument("--run_signature", type=str, default="")
    g.add_argument("--n_iters", type=int, default=10000)
    g.add_argument("--n_chains", type=int, default=128)
    g.add_argument("--energy_lamda", type=float, default=5)
    g.add_argument("--energy_function", type=str, default="product_of_experts", help="product_of_experts, supervised")
    g.add_argument("--unsupervised_expert", type=str, default="potts",
                   help="potts, transformer (= transformer-M, ESM-2 150M), transformer-S (35M), transformer-L (650M), potts+transformer")
    g.add_argument("--sampler", type=str, default="PPDE")
    g.add_argument("--nmut_threshold", type=int, default=0,
                   help="Enforce a maximum number of mutations to WT; disabled by setting to 0")
    g.add_argument("--disable_MSA_transformer_scoring", action="store_true")
    g.add_argument("--paper_results", action="store_true", default=False,
                   help="Reproduce paper results by resetting Markov chain instead of rejecting proposal")
    sa = parser.add_argument_group("simulated_annealing")
    sa.add_argument("--simulated_annealing_temp", type=float, default=0.01)
    sa.add_argument("--muts_per_seq_param", type=float, default=1.5)
    sa.add_argument("--decay_rate", type=float, default=0.999)
    ma = parser.add_argument_group("mala_approx")
    ma.add_argument("--diffusion_step_size", type=float, default=0.1)
    ma.add_argument("--diffusion_relaxation_tau", type=float, default=0.99)
    cm = parser.add_argument_group("cmaes")
    cm.add_argument("--cmaes_population_size", type=int, default=16)
    cm.add_argument("--cmaes_initial_variance", type=float, default=0.05)
    pp = parser.add_argument_group("ppde")
    pp.add_argument("--ppde_pas_length", type=int, default=2)
    pp.add_argument("--ppde_rng", type=str, default="torch", choices=["torch", "philox"],
                    help="torch: replay the reference's random stream for the same --seed; philox: device RNG (fast)")
    pp.add_argument("--ppde_seed", type=int, default=None)
    pp.add_argument("--ppde_reuse_grad", type=int, default=1)
    pp.add_argument("--ppde_shard", action="store_true", help="split the chains over the ranks of a torchrun launch")
    pp.add_argument("--ppde_timing", action="store_true", help="print one '[ppde timing] {json}' line with the wall-clock split of the run")
    pp.add_argument("--ppde_full_grad", action="store_true",
                    help="transformer experts only: let lamda * d fit/dx into the proposal gradient (the reference leaves it out)")
    pp.add_argument("--ppde_sites", type=str, default=None,
                    help="residues the sampler may mutate, e.g. '8-20,33,40-44': 0-based, inclusive, the index space of the "
                         "'min_pos max_pos' line the run prints; every other residue is frozen (default: every site of the window)")
    pp.add_argument("--ppde_exclude", type=str, default="",
                    help="letters never proposed at any open site, e.g. 'CM'. The wild-type letter of an open site is always kept")
    pp.add_argument("--ppde_library", dest="ppde_library_file", metavar="FILE", type=str, default=None,
                    help="file of lines '<pos> <letters>' ('#' comments): the letters that may be proposed at each listed residue, "
                         "unlisted residues frozen. Replaces --ppde_sites; --ppde_exclude still applies on top. The wild-type "
                         "letter of an open site is always kept")
    pp.add_argument("--ppde_reversible", action="store_true",
                    help="accept with the Metropolis-Hastings ratio of the forward proposal instead of the reference's (which scores "
                         "the reverse move at the forward index): the chains sample exp(energy)/Z over the design library (all "
                         "letters of the window when none is given), --nmut_threshold becomes a constraint instead of a reset. "
                         "Not with --paper_results")
    pp.add_argument("--ppde_betas", type=lambda t: [float(v) for v in t.split(",") if v.strip()], default=None,
                    help="parallel tempering (needs --ppde_reversible): a strictly decreasing ladder of inverse temperatures, e.g. "
                         "'1,0.7,0.5,0.35'. Consecutive chains form ensembles of one chain per rung, the chain on rung r samples "
                         "exp(beta_r energy)/Z; --n_chains must be a multiple of the number of rungs")
    pp.add_argument("--ppde_swap_every", type=int, default=1,
                    help="with --ppde_betas: neighbouring rungs of an ensemble propose to exchange their temperatures every this "
                         "many iterations (0: never)")
    pp.add_argument("--ppde_anneal_betas", type=lambda t: [float(v) for v in t.split(",") if v.strip()], default=None,
                    help="population annealing (needs --ppde_reversible; not with --ppde_betas): a non-decreasing schedule of "
                         "inverse temperatures, e.g. '0.25,0.5,1'. Every chain starts at the first; at each stage every deme is "
                         "resampled with weights exp(dbeta energy) and moves to the next. Writes anneal_parent.npy [events, n], "
                         "anneal_pre_energy.npy [events, n], anneal_log_mean_w.npy and anneal_ess.npy [events, demes] and "
                         "anneal_betas.npy; the periodic log gains a line when a stage was passed")
    pp.add_argument("--ppde_anneal_ess", type=float, default=None,
                    help="adaptive population annealing (needs --ppde_reversible; not with --ppde_anneal_betas or --ppde_betas): no "
                         "schedule; at each event every deme takes the largest step in beta whose incremental weights keep an "
                         "effective sample size of this fraction of the deme, inside (0, 1). Writes the anneal_*.npy files of "
                         "--ppde_anneal_betas with anneal_beta_path.npy [events + 1, demes] in place of anneal_betas.npy")
    pp.add_argument("--ppde_anneal_beta_start", type=float, default=None, help="with --ppde_anneal_ess: the beta every chain starts at")
    pp.add_argument("--ppde_anneal_beta_end", type=float, default=1.0, help="with --ppde_anneal_ess: the beta the demes climb to")
    pp.add_argument("--ppde_anneal_min_step", type=float, default=None,
                    help="with --ppde_anneal_ess: the smallest step in beta (default (end - start) / 4096; at least end * 2^-20)")
    pp.add_argument("--ppde_anneal_max_stages", type=int, default=4096, help="with --ppde_anneal_ess: events at most, 1..4096")
    pp.add_argument("--ppde_anneal_every", type=int, default=1,
                    help="with --ppde_anneal_betas or --ppde_anneal_ess: iterations per stage of the schedule / between two events")
    pp.add_argument("--ppde_deme", type=int, default=0,
                    help="with --ppde_anneal_betas: chains per deme, 2..1024 (0: all chains of the run); consecutive chains form a "
                         "deme, --n_chains must be a multiple of it")
    pp.add_argument("--ppde_recombine_every", type=int, default=0,
                    help="recombination (needs --ppde_reversible; not with --ppde_betas or --ppde_anneal_betas): behind every this "
                         "many iterations the chains of a deme are paired and each pair proposes to exchange a segment of open "
                         "residues (0: off). Writes recomb_partner.npy, recomb_differ.npy, recomb_outcome.npy, recomb_log_ratio.npy, "
                         "recomb_pre_energy.npy, recomb_child_energy.npy [events, n], recomb_cut.npy [events, n, 2] and "
                         "recomb_open_sites.npy; the periodic log gains a line when events happened")
    pp.add_argument("--ppde_recombine_deme", type=int, default=0,
                    help="with --ppde_recombine_every: chains per deme, even (0: all chains of the run); consecutive chains form a "
                         "deme, --n_chains must be a multiple of it")
    pp.add_argument("--ppde_sample_every", type=int, default=0,
                    help="record the population on the device after every this many iterations (0: off): samples.npy, "
                         "sample_energy.npy, sample_fitness.npy, sample_chain.npy and site_counts.npy next to the other results. "
                         "Works with either --ppde_rng")
    pp.add_argument("--ppde_sample_burn_in", type=int, default=0, help="iterations before the first recorded one is counted from")
    pp.add_argument("--ppde_sample_rung", type=int, default=None,
                    help="with --ppde_betas: the rung whose chain is recorded in every ensemble, followed through the swaps "
                         "(default 0, the beta[0] sample)")
    pp.add_argument("--ppde_sample_counts_only", action="store_true", help="keep site_counts.npy only, no per-row samples")
    pp.add_argument("--ppde_sample_pairs", metavar="SPEC", type=str, default=None,
                    help="with --ppde_sample_every: also count, on the device, how often letter a at residue i and letter b at "
                         "residue j occur together in the recorded samples: pair_counts.npy uint64 [S, 20, S, 20] and "
                         "pair_sites.npy int32 [S]. SPEC is 'all' (every residue), 'open' (the open residues of the design "
                         "library; without one the window the sampler moves in) or a site list in --ppde_sites syntax. The file "
                         "holds (20 S)^2 * 8 bytes: 29 MB at 96 sites. Kept with --ppde_sample_counts_only too")
    pp.add_argument("--ppde_archive", metavar="K", type=int, default=0,
                    help="keep, on the device, each chain's K best distinct sequences with their energies (1..32; 0: off): "
                         "archive.npy uint8 [n, K, L] with archive_energy / _fitness / _step [n, K] and archive_count [n], and the "
                         "population's distinct candidates merged from them: candidates.npy uint8 [M, L] with candidates_energy, "
                         "_fitness, _chain, _step and _nchains [M], best first. Works with either --ppde_rng; not with "
                         "--paper_results")
    pp.add_argument("--ppde_forbid", metavar="PATTERNS", type=str, default=None,
                    help="forbidden sequence patterns (needs --ppde_reversible), e.g. 'N{P}[ST],NG,K(4)': a letter, x = any, [..] a "
                         "set, {..} a complement, (n) a repetition, or a preset name (n_glycosylation, deamidation, isomerisation); "
                         "at most 32 patterns of 1..8 elements. A proposal that matches one anywhere in the sequence is rejected, so "
                         "no chain, sample or archive entry ever holds one. Sites at which the wild type matches are exempt. Writes "
                         "motif_vetoes.npy int64 [n, M] and motif_patterns.txt; the periodic log gains a 'forbidden patterns' line")
    pp.add_argument("--ppde_forbid_file", metavar="FILE", type=str, default=None,
                    help="more patterns for --ppde_forbid, one per line ('#' comments)")
    pp.add_argument("--ppde_forbid_strict", action="store_true",
                    help="with --ppde_forbid: check the sites at which the wild type matches too (a wild type that matches cannot "
                         "start a run)")
    pp.add_argument("--ppde_stats", action="store_true",
                    help="count, on the device, how the chains move: stats_iters, _accepts, _moved, _jump_sum, _dist_sum and "
                         "_wt_returns.npy int64 [n, R] per (chain, rung), stats_len_attempts and _len_accepts.npy [R, 2 pas - 1] per "
                         "(rung, path length), stats_site_changes.npy [R, L] per (rung, residue), R = rungs of the ladder or 1; the "
                         "periodic log gains an 'acceptance so far' line. Works with either --ppde_rng")
    pp.add_argument("--ppde_stats_no_sites", action="store_true", help="the statistics without stats_site_changes.npy")
    return parser


if __name__ == "__main__":
    a = build_parser().parse_args()
    a.ppde_reuse_grad = bool(a.ppde_reuse_grad)
    main(a)

"""PPDE path-auxiliary sampler driven from Python, executed by the HIP library.

`PPDE_PAS` keeps the reference's interface (ppde/protein_samplers/ppde.py:8-192): constructed from the
argparse namespace (reads ppde_pas_length, nmut_threshold, paper_results) and
    run(initial_population, num_steps, energy_function, min_pos, max_pos, oracle, log_every=50)
returns (best_x Tensor[n,L,20], best_energy np[n], best_fitness np[n], energy_history np[T+1,n],
fitness_history np[T+1,n], random_traj list of T+1 np[L,20]); with ONE chain fitness_history is (T+1,) as in the reference
(ppde.py:178-183, nets.py:442; fixture run_toy24_n1.npz).

Extra, optional attributes on `args` (absent in the reference, defaults keep its behaviour):
    ppde_rng            'torch' (default): path lengths / race variates / accept uniforms are drawn with torch's
                        CPU generator in the reference's order, so a run replays the reference's trajectory for the
                        same torch.manual_seed; 'philox': counter-based device RNG (the fast path).
    ppde_seed           Philox key (default: args.seed or torch.initial_seed()).
    ppde_reuse_grad     True (default): energy/gradient of the current state are carried over from the previous
                        iteration instead of being recomputed (bit-identical results).
    ppde_use_graph      True (default): replay iterations from a captured hipGraph in philox mode.
    ppde_streams        1 (default). >1: philox mode cuts the chains into this many sub-populations whose iterations run on
                        separate HIP streams and overlap on the GPU (independent chains: results unchanged).
    ppde_cpu_alias      False (default): state histories hold the pre-reset state (reference on cuda);
                        True reproduces the reference's `--device cpu` aliasing artefact.
    ppde_library        None (default), or a design library: uint32 [L] / bool [L, 20] of the letters that may be proposed at
                        each residue (ppde_amd/library.py). Enforced exactly inside the proposal kernels; every site outside
                        [min_pos, max_pos] is frozen in it and the chains run over the full range, so nothing in such a run
                        relies on the range mask (which leaks 2^-23 per masked entry, as in the reference). Every rank of a
                        sharded run passes the same library.
    ppde_reversible     False (default): the reference's accept ratio, whose stationary law is not exp(energy)/Z (it scores the
                        reverse move at the index the forward move chose, ppde.py:128-132). True: a Metropolis-Hastings step of the
                        same forward proposal (include/ppde_hip.h, ppde_chains_set_reversible): the chains sample
                        exp(energy) / Z over the library, with nmut_threshold as a constraint (dist < threshold) instead of a
                        reset. Such a run always has a library (all letters over [min_pos, max_pos] when none is given), so the
                        restriction is hard; paper_results and an initial population outside the library are refused.
    ppde_betas          None (default), or a ladder of inverse temperatures beta[0] > beta[1] > ... > 0: parallel tempering of a
                        reversible run (include/ppde_hip.h, ppde_chains_set_tempering). Consecutive chains form ensembles of
                        len(ppde_betas); the chain on rung r samples exp(beta_r energy)/Z and neighbouring rungs propose to
                        exchange temperatures every ppde_swap_every iterations (default 1; 0: never). Needs ppde_reversible; the
                        population (and every shard boundary) must be a multiple of the ladder; not with ppde_streams > 1.
                        Histories and best states stay on the untempered energy. After run(), `sampler.tempering` holds
                        betas, rung_history [T+1, n], swap_attempts and swap_accepts [n / R, R - 1].
    ppde_anneal_betas   None (default), or a schedule of inverse temperatures beta[0] <= beta[1] <= ... <= beta[S]: population
                        annealing of a reversible run (include/ppde_hip.h, ppde_chains_set_annealing). Consecutive chains form
                        demes of ppde_deme (default 0: all chains of the run); every chain starts at beta[0], and behind every
                        ppde_anneal_every-th iteration (default 1) each deme is resampled with weights exp(dbeta energy) and moves
                        to the next beta. Needs ppde_reversible; not with ppde_betas, not with ppde_streams > 1; the population
                        (and every shard boundary) must be a multiple of the deme. Histories and best states stay on the
                        untempered energy. After run(), `sampler.annealing` holds betas, deme, every, parent [events, n] (GLOBAL
                        chain index of the ancestor), pre_energy [events, n], log_mean_w and ess [events, n / deme], beta_now [n]
                        and `summary` (ppde_amd/anneal.py: summarise).
    ppde_anneal_ess     None (default): off. rho in (0, 1): ADAPTIVE population annealing (include/ppde_hip.h,
                        ppde_chains_set_annealing_adaptive) in place of a schedule: every deme starts at ppde_anneal_beta_start
                        and behind every ppde_anneal_every-th iteration takes the largest step towards ppde_anneal_beta_end
                        (default 1) that keeps the ESS of its incremental weights at rho times the deme, at least
                        ppde_anneal_min_step (default (end - start) / 4096), for at most ppde_anneal_max_stages events (default
                        4096). ppde_deme and the conditions of ppde_anneal_betas apply; not together with ppde_anneal_betas.
                        `sampler.annealing` then holds betas = (start, end), ess_target, min_step, max_stages, the same arrays and
                        beta_path [events + 1, n / deme], the inverse temperature of every deme before the first and after each
                        event; its summary adds arrived and stages per deme.
    ppde_recombine_every 0 (default): off. k > 0: behind every k-th iteration the chains of each deme of ppde_recombine_deme
                        consecutive chains (default 0: all chains of the run; even) are paired and every pair proposes to exchange
                        a segment of open residues, accepted by Metropolis on the pair (include/ppde_hip.h,
                        ppde_chains_set_recombination). Needs ppde_reversible; not with ppde_betas, ppde_anneal_betas,
                        paper_results or ppde_streams > 1; the population (and every shard boundary) must be a multiple of the
                        deme. After run(), `sampler.recombination` holds deme, every, open_sites, events, partner (GLOBAL chain
                        index), lo, hi, cut [events, n, 2], differ, child_dist, outcome, log_ratio, pre_energy, child_energy
                        [events, n] and `summary` (ppde_amd/recombine.py: summarise; lineage gives the mosaic of founders).
    ppde_sample_every   0 (default): off. k > 0: the population after every k-th iteration (counted from ppde_sample_burn_in,
                        default 0) is recorded on the device (include/ppde_hip.h, ppde_chains_set_recorder): no host round trip,
                        nothing else of the run changes. With a ladder the recorder follows rung ppde_sample_rung (default 0, the
                        beta[0] chain of every ensemble, wherever the swaps have moved it); without one every chain is a slot.
                        ppde_sample_counts_only keeps the per-site letter counts only. After run(), `sampler.samples` holds idx
                        uint8 [rows, slots, L], energy / fitness [rows, slots], chain int [rows, slots] (GLOBAL chain index),
                        site_counts uint64 [L, 20] and rows; a sharded run gathers the slots in global order and sums the counts.
                        Not with ppde_streams > 1.
    ppde_sample_pairs   None or '' (default): off. With ppde_sample_every > 0: pairwise letter co-occurrence counts of the same
                        recorded rows and slots (include/ppde_hip.h, ppde_chains_set_pair_counts), kept with
                        ppde_sample_counts_only too. 'all': every residue; 'open': the open residues of the run's library
                        (without one: min_pos..max_pos); a site list in library.parse_sites syntax ('8-20,33') or a strictly
                        increasing sequence of 0-based residues. After run(), `sampler.samples` also holds pair_counts uint64
                        [S, 20, S, 20] and pair_sites int32 [S] (both None when off); a sharded run sums the counts.
    ppde_forbid         None (default): off. Forbidden sequence patterns, as text 'N{P}[ST], NG, K(4)' (ppde_amd/motifs.py: a letter, x
                        = any, [..] a set, {..} a complement, (n) a repetition; a name of motifs.PRESETS stands for its pattern), a
                        list of such strings or a motifs.Patterns: at most 32 patterns of 1..8 elements. A proposal that matches one
                        anywhere in the sequence (frozen residues are context) is rejected on the device, so the chains sample
                        exp(E) 1[free] / Z (include/ppde_hip.h, ppde_chains_set_forbidden_patterns). Needs ppde_reversible. Sites at
                        which the wild type matches are exempt unless ppde_forbid_strict is set. Every initial state must be free.
                        After run(), `sampler.forbidden` holds text, allow_native, active uint32 [L], vetoes int64 [n, M] (global
                        chain order) and `summary` (motifs.summarise: the share of proposals vetoed, overall and per pattern).
    ppde_forbid_strict  False (default). True: the wild type's own matches are checked too (allow_native = 0).
    ppde_archive        None or 0 (default): off. K in 1..32: every chain keeps, on the device, the K best distinct sequences it
                        visited, each with its own energy (include/ppde_hip.h, ppde_chains_set_archive): n K L bytes whatever the
                        run length, no host round trip, nothing else of the run changes. The wild type is never archived. After
                        run(), `sampler.archive` holds idx uint8 [n, K, L] (255 beyond count), energy / fitness [n, K], step
                        [n, K], count [n], chain [n] (GLOBAL chain index) and `candidates`, the population's distinct sequences
                        merged from them (ppde_amd/archive.py: idx, energy, fitness, chain, step, n_chains; best first). A sharded
                        run gathers the per-chain archives in global chain order and merges on every rank. Not with
                        paper_results, not with ppde_streams > 1.
    ppde_stats          None or False (default): off. True: move statistics counted on the device (include/ppde_hip.h,
                        ppde_chains_set_stats): acceptances, jump distances, mutation counts and wild-type returns per (chain,
                        rung), attempts and acceptances per (rung, path length), changes per (rung, residue); no host round trip,
                        nothing else of the run changes. 'no-sites' leaves the per-residue counts out. After run(),
                        `sampler.stats` holds the raw int64 arrays (ppde_amd/stats.py: KEYS), chain [n] (GLOBAL chain index), betas
                        and `summary` (stats.summarise). A sharded run gathers the per-chain arrays in global chain order and sums
                        the others; the periodic log gains one line. Not with ppde_streams > 1.
    ppde_shard          False (default). True with torch.distributed initialised: chains are split over ranks
                        and gathered at the end (one RCCL all_gather); every rank returns the full result.
"""
import ctypes as C
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip, motifs as chain_motifs, anneal as chain_anneal, recombine as chain_recombine, archive as chain_archive, library as design_library, stats as chain_stats
from .base_sampler import BaseSampler
from .encoding import idx_to_onehot
from .noise import draw_chunk
from .parallel import Shard, active as collectives_active, agree_from_rank0, boundary_cut, world


def recorder_rows(max_steps, burn_in, every):
    """Row capacity of a recorder over max_steps iterations (include/ppde_hip.h): (max_steps - burn_in) / every."""
    return (max_steps - burn_in) // every if max_steps > burn_in else 0


def recorder_row_of(t, burn_in, every):
    """Row that holds the state after t completed iterations, or None when that iteration is not recorded."""
    d = t - burn_in
    return d // every - 1 if d > 0 and d % every == 0 else None


def recorder_rows_done(steps_done, burn_in, every):
    return recorder_rows(steps_done, burn_in, every)


def check_pair_spec(spec):
    """ppde_sample_pairs as None (off), 'all', 'open', a site-list string, or a strictly increasing tuple of residues; ValueError
    otherwise. Whether the residues lie inside the sequence is checked by pair_sites_of, once its length is known."""
    if spec is None or (isinstance(spec, str) and spec.strip() == ""):
        return None
    if isinstance(spec, str):
        word = spec.strip()
        if word.lower() in ("all", "open"):
            return word.lower()
        try:
            design_library.parse_sites(word, 1 << 30)         # (syntax only)
        except ValueError as e:
            raise ValueError(f"ppde_sample_pairs: {e} (or 'all', 'open')") from None
        return word
    try:
        sites = tuple(int(v) for v in spec)
        exact = all(float(v) == int(v) for v in spec)
    except (TypeError, ValueError):
        raise ValueError(f"ppde_sample_pairs: expected 'all', 'open', a site list like '8-20,33' or a sequence of residues, got {spec!r}") from None
    if not exact or not sites:
        raise ValueError(f"ppde_sample_pairs: a sequence of residues must hold at least one whole number, got {spec!r}")
    if sites[0] < 0 or any(b <= a for a, b in zip(sites, sites[1:])):
        raise ValueError(f"ppde_sample_pairs: residues must be >= 0 and strictly increasing, got {spec!r}")
    return sites


def pair_sites_of(spec, L, min_pos, max_pos, lib_words=None):
    """The residues a checked ppde_sample_pairs selects in a sequence of L: None for every residue, else int32 [S]."""
    if spec == "all":
        return None
    if spec == "open":
        if lib_words is not None:
            return design_library.open_sites(lib_words).astype(np.int32)
        return np.arange(int(min_pos), int(max_pos) + 1, dtype=np.int32)
    if isinstance(spec, str):
        try:
            return np.asarray(design_library.parse_sites(spec, L), np.int32)
        except ValueError as e:
            raise ValueError(f"ppde_sample_pairs: {e}") from None
    if spec[-1] >= L:
        raise ValueError(f"ppde_sample_pairs: residue {spec[-1]} lies outside the sequence 0..{L - 1}")
    return np.asarray(spec, np.int32)


def check_forbid(spec, strict=False, reversible=False, paper_results=False):
    """(Patterns or None, allow_native) of the ppde_forbid* arguments; ValueError for what the ABI would refuse and can be seen
    without the sequence (the text form, the number of patterns and their lengths, the modes)."""
    strict = bool(strict)
    if spec is None or (isinstance(spec, (str, list, tuple)) and len(spec) == 0):
        if strict:
            raise ValueError("ppde_forbid_strict needs ppde_forbid")
        return None, True
    if not reversible:
        raise ValueError("ppde_forbid: a pattern constraint needs ppde_reversible (only there is the target exp(E) 1[free] / Z that "
                         "the explicit rejection keeps)" + ("; paper_results excludes it" if paper_results else ""))
    return chain_motifs.parse(spec), not strict


def check_forbid_population(pt, allow_native, wt_idx, population_idx):
    """What needs the sequence: the setter's checks against L, at least one active (pattern, position), and every initial state
    free; ValueError names the chain, the pattern and the position."""
    L = int(np.asarray(wt_idx).size)
    chain_motifs.check_patterns(pt, L)
    if not chain_motifs.active_mask(pt, L, wt_idx, allow_native).any():
        raise ValueError("ppde_forbid: no active (pattern, position): the wild type matches every pattern at every start")
    fp, pos = chain_motifs.find(population_idx, pt, wt_idx, allow_native)
    bad = np.flatnonzero(fp >= 0)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"ppde_forbid: the initial state of chain {b} is not free: forbidden pattern {int(fp[b])} ({pt.text[int(fp[b])]}) "
                         f"matches at position {int(pos[b])}" + ("" if allow_native else " (ppde_forbid_strict checks the wild type's own sites)"))


def check_archive(k, paper_results=False, n_streams=1):
    """ppde_archive as 0 (off: None or 0) or K in 1..32; ValueError otherwise, and for what an archive cannot be combined with."""
    if k is None or (not isinstance(k, bool) and k == 0):
        return 0
    try:
        whole = not isinstance(k, bool) and float(k) == int(k) and 1 <= int(k) <= 32
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError(f"ppde_archive: K must be a whole number in 1..32 (None or 0: off), got {k!r}")
    if paper_results:
        raise ValueError("ppde_archive: paper_results is not supported (after a rejection its history row holds the energy of the "
                         "state that was left while the chain continues from its initial state)")
    if int(n_streams) > 1:
        raise ValueError("ppde_archive: ppde_streams > 1 is not supported (one launch archives every chain)")
    return int(k)


def check_stats(spec, n_streams=1):
    """ppde_stats as None (off: None or False), True, or 'no-sites'; ValueError otherwise, and for what statistics cannot be
    combined with."""
    if spec is None or spec is False:
        return None
    if spec is not True and spec != "no-sites":
        raise ValueError(f"ppde_stats: expected None / False (off), True or 'no-sites', got {spec!r}")
    if int(n_streams) > 1:
        raise ValueError("ppde_stats: ppde_streams > 1 is not supported (the counters have one owner per launch)")
    return spec


def check_ladder(betas):
    """A tempering ladder as fp32 [R], or ValueError: 1..64 finite, positive, strictly decreasing inverse temperatures."""
    b = np.asarray(betas, dtype=np.float32).reshape(-1)
    if not 1 <= b.size <= 64:
        raise ValueError(f"ppde_betas: a ladder has 1 to 64 rungs, got {b.size}")
    if not np.isfinite(b).all():
        raise ValueError("ppde_betas: every beta must be finite")
    if not (b > 0).all():
        raise ValueError("ppde_betas: every beta must be positive")
    if not (b[1:] < b[:-1]).all():
        raise ValueError("ppde_betas: the ladder must be strictly decreasing")
    return np.ascontiguousarray(b)


def check_tempering(betas, swap_every, reversible, n_streams):
    """(ladder fp32 [R] or None, swap_every) of the ppde_betas / ppde_swap_every arguments; ValueError for what the ABI would refuse
    and can be seen without the population."""
    ladder = None if betas is None or len(betas) == 0 else check_ladder(betas)
    swap_every = int(swap_every)
    if ladder is not None:
        if not reversible:
            raise ValueError("ppde_betas: tempering needs ppde_reversible (only there is the law at beta, exp(beta energy)/Z, defined)")
        if swap_every < 0:
            raise ValueError("ppde_swap_every must be >= 0")
        if int(n_streams) > 1:
            raise ValueError("ppde_betas: ppde_streams > 1 is not supported (the swap couples the chains of an ensemble)")
    return ladder, swap_every


def check_schedule(betas):
    """An annealing schedule as fp32 [S + 1], or ValueError: 2..4097 finite, positive, non-decreasing inverse temperatures."""
    b = np.asarray(betas, dtype=np.float32).reshape(-1)
    if not 2 <= b.size <= 4097:
        raise ValueError(f"ppde_anneal_betas: a schedule has 1 to 4096 stages (2 to 4097 betas), got {b.size} betas")
    if not np.isfinite(b).all():
        raise ValueError("ppde_anneal_betas: every beta must be finite")
    if not (b > 0).all():
        raise ValueError("ppde_anneal_betas: every beta must be positive")
    if not (b[1:] >= b[:-1]).all():
        raise ValueError("ppde_anneal_betas: the schedule must not decrease")
    return np.ascontiguousarray(b)


def check_annealing(betas, every, deme, reversible, ladder, n_streams):
    """(schedule fp32 [S + 1] or None, every, deme) of the ppde_anneal_* arguments; ValueError for what the ABI would refuse and
    can be seen without the population (deme 0 = all chains of the run, resolved there)."""
    if betas is None or len(betas) == 0:
        return None, int(every), int(deme)
    sched = check_schedule(betas)
    if not reversible:
        raise ValueError("ppde_anneal_betas: annealing needs ppde_reversible (only there is the law at beta, exp(beta energy)/Z, defined)")
    if ladder is not None:
        raise ValueError("ppde_anneal_betas: a schedule and a ladder (ppde_betas) cannot be combined")
    if int(every) < 1:
        raise ValueError("ppde_anneal_every must be >= 1")
    if int(deme) != 0 and not 2 <= int(deme) <= 1024:
        raise ValueError("ppde_deme must be in 2..1024 (0: all chains of the run)")
    if int(n_streams) > 1:
        raise ValueError("ppde_anneal_betas: ppde_streams > 1 is not supported (the selection couples the chains of a deme)")
    return sched, int(every), int(deme)


def check_annealing_adaptive(ess, beta_start, beta_end, min_step, max_stages, every, deme, betas, reversible, ladder, n_streams):
    """None (ess None: off), or dict(ess_target, beta_start, beta_end, min_step, max_stages) of the adaptive ppde_anneal_*
    arguments in fp32 (min_step None: (beta_end - beta_start) / 4096); ValueError for what the ABI would refuse and can be seen
    without the population."""
    if ess is None:
        return None
    if betas is not None and len(betas) > 0:
        raise ValueError("ppde_anneal_ess: an ESS target and a schedule (ppde_anneal_betas) cannot be combined")
    if not reversible:
        raise ValueError("ppde_anneal_ess: annealing needs ppde_reversible (only there is the law at beta, exp(beta energy)/Z, defined)")
    if ladder is not None:
        raise ValueError("ppde_anneal_ess: annealing and a ladder (ppde_betas) cannot be combined")
    if beta_start is None:
        raise ValueError("ppde_anneal_ess needs ppde_anneal_beta_start")
    rho, b0, b1 = np.float32(ess), np.float32(beta_start), np.float32(1.0 if beta_end is None else beta_end)
    if not (np.isfinite(rho) and 0 < rho < 1):
        raise ValueError("ppde_anneal_ess must be inside (0, 1)")
    if not (np.isfinite(b0) and np.isfinite(b1) and b0 > 0 and b1 > 0):
        raise ValueError("ppde_anneal_beta_start and ppde_anneal_beta_end must be finite and positive")
    if not b0 < b1:
        raise ValueError("ppde_anneal_beta_start must be below ppde_anneal_beta_end")
    step = np.float32((float(b1) - float(b0)) / 4096.0) if min_step is None else np.float32(min_step)
    if not (np.isfinite(step) and step >= b1 * np.float32(2.0 ** -20)):
        raise ValueError("ppde_anneal_min_step must be finite and >= ppde_anneal_beta_end * 2^-20 (a step that changes beta in fp32)")
    stages = 4096 if max_stages is None else int(max_stages)
    if not 1 <= stages <= 4096:
        raise ValueError("ppde_anneal_max_stages must be in 1..4096")
    if int(every) < 1:
        raise ValueError("ppde_anneal_every must be >= 1")
    if int(deme) != 0 and not 2 <= int(deme) <= 1024:
        raise ValueError("ppde_deme must be in 2..1024 (0: all chains of the run)")
    if int(n_streams) > 1:
        raise ValueError("ppde_anneal_ess: ppde_streams > 1 is not supported (the selection couples the chains of a deme)")
    return dict(ess_target=float(rho), beta_start=float(b0), beta_end=float(b1), min_step=float(step), max_stages=stages)


def check_demes(n_global, deme, num_steps, every, n_stages, shard_starts=(0,)):
    """The deme size of a run of n_global chains (deme 0: all of them), or ValueError: a size outside 2..1024, a population or a
    shard boundary that cuts a deme, a run too short for one event."""
    D = int(n_global) if int(deme) == 0 else int(deme)
    if not 2 <= D <= 1024:
        raise ValueError(f"ppde_deme: a deme has 2 to 1024 chains, got {D}" + (" (ppde_deme 0 = all chains of the run)" if int(deme) == 0 else ""))
    if n_global % D:
        raise ValueError(f"ppde_deme: the population of {n_global} chains is no multiple of the deme of {D}")
    cut = boundary_cut(shard_starts, D)
    if cut:
        raise ValueError(f"ppde_deme: the shard boundary at chain {cut[1]} (rank {cut[0]} of {len(shard_starts)}) cuts a deme of {D} chains")
    if min(int(n_stages), int(num_steps) // int(every)) == 0:
        raise ValueError(f"ppde_anneal_every: no event fits into {int(num_steps)} iterations (every {int(every)})")
    return D


def check_recombination(every, deme, reversible, ladder, schedule, paper_results, n_streams):
    """(every, deme) of the ppde_recombine_* arguments (every 0: off; deme 0 = all chains of the run, resolved with the
    population); ValueError for what the ABI would refuse and can be seen without the population."""
    every, deme = int(every or 0), int(deme or 0)
    if every < 0:
        raise ValueError("ppde_recombine_every must be >= 0 (0: no recombination)")
    if every == 0:
        if deme:
            raise ValueError("ppde_recombine_deme needs ppde_recombine_every > 0")
        return 0, 0
    if not reversible:
        raise ValueError("ppde_recombine_every: recombination needs ppde_reversible (only there do the chains have the law whose "
                         "product the exchange keeps)")
    if ladder is not None or schedule is not None:
        raise ValueError("ppde_recombine_every: recombination cannot be combined with a ladder (ppde_betas) or a schedule "
                         "(ppde_anneal_betas): its decision takes no beta per chain")
    if paper_results:
        raise ValueError("ppde_recombine_every: paper_results is not supported")
    if deme < 0 or deme % 2:
        raise ValueError("ppde_recombine_deme must be even and >= 2 (0: all chains of the run)")
    if int(n_streams) > 1:
        raise ValueError("ppde_recombine_every: ppde_streams > 1 is not supported (the exchange couples the chains of a deme)")
    return every, deme


def check_recombination_demes(n_global, deme, num_steps, every, shard_starts=(0,)):
    """The deme size of a recombination run of n_global chains (deme 0: all of them), or ValueError: an odd size, a population or
    a shard boundary that cuts a deme, a run too short for one event."""
    D = int(n_global) if int(deme) == 0 else int(deme)
    if D < 2 or D % 2:
        raise ValueError(f"ppde_recombine_deme: a deme has an even number of chains, at least 2, got {D}" +
                         (" (ppde_recombine_deme 0 = all chains of the run)" if int(deme) == 0 else ""))
    if n_global % D:
        raise ValueError(f"ppde_recombine_deme: the population of {n_global} chains is no multiple of the deme of {D}")
    cut = boundary_cut(shard_starts, D)
    if cut:
        raise ValueError(f"ppde_recombine_deme: the shard boundary at chain {cut[1]} (rank {cut[0]} of {len(shard_starts)}) cuts a "
                         f"deme of {D} chains")
    if int(num_steps) // int(every) == 0:
        raise ValueError(f"ppde_recombine_every: no event fits into {int(num_steps)} iterations (every {int(every)})")
    return D


def check_recorder(every, burn_in, rung, counts_only, pairs, ladder, n_streams):
    """(every, burn_in, rung, counts_only, pairs) of the ppde_sample_* arguments (every 0: no recorder; rung None without a ladder,
    default 0 with one; pairs as check_pair_spec); ValueError for what the ABI would refuse and can be seen without the run length."""
    every, burn_in, counts_only = int(every or 0), int(burn_in or 0), bool(counts_only)
    pairs = check_pair_spec(pairs)
    if pairs is not None and every <= 0:
        raise ValueError("ppde_sample_pairs needs ppde_sample_every > 0 (pair counts follow the recorder's schedule)")
    if every < 0:
        raise ValueError("ppde_sample_every must be >= 0 (0: no recorder)")
    if every == 0 and (burn_in or rung is not None or counts_only):
        raise ValueError("ppde_sample_burn_in / ppde_sample_rung / ppde_sample_counts_only need ppde_sample_every > 0")
    if every:
        if burn_in < 0:
            raise ValueError("ppde_sample_burn_in must be >= 0")
        if int(n_streams) > 1:
            raise ValueError("ppde_sample_every: ppde_streams > 1 is not supported (the recorder's counters have one owner per launch)")
        if ladder is None:
            if rung is not None:
                raise ValueError("ppde_sample_rung: following a rung needs a ladder (ppde_betas)")
        else:
            rung = 0 if rung is None else int(rung)
            if not 0 <= rung < ladder.size:
                raise ValueError(f"ppde_sample_rung must be a rung of the ladder, 0..{ladder.size - 1}")
    return every, burn_in, rung, counts_only, pairs


class Chains:
    """Owner of a `ppde_chains` (include/ppde_hip.h)."""

    def __init__(self, model, n_chains, max_steps, pas_length, nmut_threshold, paper_results, min_pos, max_pos, which,
                 rng_mode, reuse_grad=True, record_after_reset=False, trace=False, random_chain=-1, use_graph=True,
                 seed=0, chain_offset=0, n_streams=1):
        self.model, self.lib = model, model.lib
        self.n, self.T, self.mu_max = int(n_chains), int(max_steps), 2 * int(pas_length) - 1
        self.cfg = _hip.ChainConfig(
            n_chains=self.n, max_steps=self.T, pas_length=int(pas_length), nmut_threshold=int(nmut_threshold),
            paper_results=int(bool(paper_results)), min_pos=int(min_pos), max_pos=int(max_pos), which=int(which),
            rng_mode=int(rng_mode), reuse_grad=int(bool(reuse_grad)), record_after_reset=int(bool(record_after_reset)),
            trace=int(bool(trace)), random_chain=int(random_chain), use_graph=int(bool(use_graph)), n_streams=int(n_streams),
            seed=int(seed) & (2 ** 64 - 1), chain_offset=int(chain_offset))
        self.handle = C.c_void_p()
        with torch.cuda.device(model.device):
            _hip.check(self.lib.ppde_chains_create(C.byref(self.handle), model.handle, C.byref(self.cfg)))

    def _call(self, name, *args):
        """ppde_chains_<name>(handle, *args) on the model's device; a non-zero status raises (_hip.check)."""
        with torch.cuda.device(self.model.device):
            _hip.check(getattr(self.lib, "ppde_chains_" + name)(self.handle, *args))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.ppde_chains_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_library(self, mask):
        """Design library for the forward proposals: uint32 [L] (bit k = letter k allowed, 0 = frozen) or bool [L, 20]; None
        clears it. Only before init() (the graphs captured there hold the device copy's address)."""
        words = None if mask is None else design_library.as_words(mask, self.model.L)
        self._call("set_library", _hip.ptr(words))
        self.library = words

    def set_reversible(self, on=True):
        """Reversible mode (include/ppde_hip.h, ppde_chains_set_reversible): the accept phase scores the moves that undo the
        path under the forward row function, so the chains sample exp(energy)/Z over the library. Only before init()."""
        self._call("set_reversible", int(bool(on)))
        self.reversible = bool(on)

    def set_tempering(self, betas, swap_every=1):
        """Parallel tempering (include/ppde_hip.h, ppde_chains_set_tempering): a ladder betas[0] > betas[1] > ... > 0 over
        ensembles of len(betas) consecutive chains, replica exchange every `swap_every` iterations (0: never). None or an
        empty ladder clears it. Needs reversible mode; only before init()."""
        ladder = None if betas is None or len(betas) == 0 else np.ascontiguousarray(np.asarray(betas, dtype=np.float32).reshape(-1))
        self._call("set_tempering", 0 if ladder is None else int(ladder.size), _hip.ptr(ladder), int(swap_every))
        self.betas, self.swap_every = ladder, int(swap_every)

    def tempering_state(self):
        """rung int32 [n] and beta fp32 [n] each chain holds now, swap_attempts / swap_accepts int64 [n / R, R - 1]."""
        R = 0 if getattr(self, "betas", None) is None else int(self.betas.size)
        pairs = (self.n // R, R - 1) if R else (0, 0)
        out = dict(rung=np.empty(self.n, np.int32), beta=np.empty(self.n, np.float32),
                   swap_attempts=np.zeros(pairs, np.int64), swap_accepts=np.zeros(pairs, np.int64))
        self._call("tempering_state", *[_hip.ptr(out[k]) for k in ("rung", "beta", "swap_attempts", "swap_accepts")])
        return out

    def tempering_history(self):
        """uint8 [steps_done + 1, n]: the rung each chain held after every iteration (row 0: the start)."""
        out = np.empty((self.steps_done + 1, self.n), np.uint8)
        self._call("tempering_history", _hip.ptr(out))
        return out

    def set_annealing(self, betas, every=1, deme=None):
        """Population annealing (include/ppde_hip.h, ppde_chains_set_annealing): a schedule betas[0] <= ... <= betas[S] over demes
        of `deme` consecutive chains (None: all chains of the object), one stage behind every `every`-th iteration. None or an
        empty schedule clears it. Needs reversible mode; only before init()."""
        if betas is None or len(betas) == 0:
            self._call("set_annealing", None)
            self.anneal = None
            return
        sched = np.ascontiguousarray(np.asarray(betas, dtype=np.float32).reshape(-1))
        D = self.n if deme is None else int(deme)
        cfg = _hip.AnnealConfig(deme=D, every=int(every), n_stages=int(sched.size) - 1,
                                beta=sched.ctypes.data_as(C.POINTER(C.c_float)))
        self._call("set_annealing", C.byref(cfg))
        self.anneal = dict(betas=sched, every=int(every), deme=D)

    def set_annealing_adaptive(self, beta_start, beta_end, ess_target, every=1, deme=None, max_stages=4096, min_step=None):
        """Adaptive population annealing (include/ppde_hip.h, ppde_chains_set_annealing_adaptive): every deme of `deme` consecutive
        chains (None: all chains of the object) starts at beta_start and, behind every `every`-th iteration, takes the largest
        step towards beta_end that keeps the ESS of its incremental weights at ess_target times the deme -- at least min_step
        (None: (beta_end - beta_start) / 4096), for at most max_stages events. beta_start None clears the mode. Replaces a fixed
        schedule and is replaced by one. Needs reversible mode; only before init()."""
        if beta_start is None:
            self._call("set_annealing_adaptive", None)
            self.anneal = None
            return
        b0, b1 = np.float32(beta_start), np.float32(beta_end)
        step = np.float32((float(b1) - float(b0)) / 4096.0) if min_step is None else np.float32(min_step)
        D = self.n if deme is None else int(deme)
        cfg = _hip.AnnealAdaptiveConfig(deme=D, every=int(every), max_stages=int(max_stages), beta_start=float(b0), beta_end=float(b1),
                                        ess_target=float(ess_target), min_step=float(step))
        self._call("set_annealing_adaptive", C.byref(cfg))
        self.anneal = dict(betas=np.array([b0, b1], np.float32), every=int(every), deme=D, adaptive=True,
                           ess_target=float(np.float32(ess_target)), min_step=float(step), max_stages=int(max_stages))

    def annealing_shape(self):
        """(deme size, event capacity, events that have happened)."""
        d, cap, done = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("annealing_shape", C.byref(d), C.byref(cap), C.byref(done))
        return d.value, cap.value, done.value

    def annealing_state(self, first=0, count=None):
        """Events [first, first + count) (default: all so far): parent int32 [count, n] (local index of the ancestor), pre_energy
        fp32 [count, n], log_mean_w / ess fp64 [count, n / D]; beta_before / beta_after fp32 [count, n / D], the inverse temperature
        of every deme around each event; beta fp32 [n] each chain holds now; events = how many have happened."""
        D, _, done = self.annealing_shape()
        first = int(first)
        count = done - first if count is None else int(count)
        k = max(count, 0)
        out = dict(parent=np.empty((k, self.n), np.int32), pre_energy=np.empty((k, self.n), np.float32),
                   log_mean_w=np.empty((k, self.n // D), np.float64), ess=np.empty((k, self.n // D), np.float64),
                   beta=np.empty(self.n, np.float32), beta_before=np.empty((k, self.n // D), np.float32),
                   beta_after=np.empty((k, self.n // D), np.float32))
        self._call("annealing_read", first, count, *[_hip.ptr(out[k_]) for k_ in ("parent", "pre_energy", "log_mean_w", "ess", "beta")])
        self._call("annealing_read_betas", first, count, _hip.ptr(out["beta_before"]), _hip.ptr(out["beta_after"]))
        out["events"] = done
        return out

    RECOMBINATION_FIELDS = (("partner", np.int32), ("lo", np.int32), ("hi", np.int32), ("differ", np.int32), ("child_dist", np.int32),
                            ("outcome", np.uint8), ("log_ratio", np.float32), ("pre_energy", np.float32), ("child_energy", np.float32))

    def set_recombination(self, every, deme=0):
        """Recombination (include/ppde_hip.h, ppde_chains_set_recombination): behind every `every`-th iteration the chains of each
        deme of `deme` consecutive chains (0 or None: all chains of the object) are paired and every pair proposes to exchange a
        segment of open residues. every None or 0 clears it. Needs reversible mode; only before init() and after set_library()."""
        if not every:
            self._call("set_recombination", None)
            self.recombination = None
            return
        D = self.n if not deme else int(deme)
        cfg = _hip.RecombineConfig(deme=D, every=int(every))
        self._call("set_recombination", C.byref(cfg))
        self.recombination = dict(every=int(every), deme=D)

    def recombination_shape(self):
        """(deme size, open residues int32 [S_o], event capacity, events that have happened)."""
        d, n_open, cap, done = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._call("recombination_shape", C.byref(d), C.byref(n_open), None, C.byref(cap), C.byref(done))
        sites = np.empty(n_open.value, np.int32)
        self._call("recombination_shape", None, None, _hip.ptr(sites), None, None)
        return d.value, sites, cap.value, done.value

    def recombination_state(self, first=0, count=None):
        """Events [first, first + count) (default: all so far), [count, n] each: partner (LOCAL index), lo, hi (indices into
        open_sites), differ, child_dist int32, outcome uint8 (0 rejected by u, 1 accepted, 2 a child at the mutation cap, 3 a
        non-finite child energy, 4 a child that matches a forbidden pattern), log_ratio, pre_energy, child_energy fp32; deme,
        every, open_sites, events."""
        D, sites, _, done = self.recombination_shape()
        first = int(first)
        count = done - first if count is None else int(count)
        out = {k_: np.empty((max(count, 0), self.n), t) for k_, t in self.RECOMBINATION_FIELDS}
        self._call("recombination_read", first, count, *[_hip.ptr(out[k_]) for k_, _ in self.RECOMBINATION_FIELDS])
        out.update(deme=D, every=self.recombination["every"], open_sites=sites, events=done)
        return out

    def set_forbidden(self, patterns, allow_native=True):
        """Forbidden patterns (include/ppde_hip.h, ppde_chains_set_forbidden_patterns): `patterns` as ppde_amd/motifs.py parses
        them ('N{P}[ST], NG', a list, or Patterns); a proposal that matches one at an active start is rejected, so the chains
        sample the target restricted to free states. allow_native exempts the sites at which the wild type matches. None clears
        it. Needs reversible mode; only before init(). `self.forbidden["note"]` holds what the setter had to say (a wild type
        that is not free under allow_native False)."""
        if patterns is None:
            self._call("set_forbidden_patterns", None)
            self.forbidden = None
            return
        cfg, pt = chain_motifs.config(patterns, allow_native)
        self._call("set_forbidden_patterns", C.byref(cfg))
        note = self.lib.ppde_last_error().decode()
        self.forbidden = dict(patterns=pt, allow_native=bool(allow_native),
                              note=note if note.startswith("ppde_chains_set_forbidden_patterns: note:") else None)

    def forbidden_state(self):
        """dict(n_patterns, allow_native, active uint32 [L], text, vetoes int64 [n, M] -- None before init())."""
        M, an = C.c_int32(), C.c_int32()
        active = np.empty(self.model.L, np.uint32)
        self._call("forbidden_shape", C.byref(M), C.byref(an), _hip.ptr(active))
        vetoes = None
        if getattr(self, "_initialised", False):
            vetoes = np.zeros((self.n, M.value), np.int64)
            self._call("forbidden_read", _hip.ptr(vetoes))
        return dict(n_patterns=M.value, allow_native=bool(an.value), active=active, text=list(self.forbidden["patterns"].text),
                    vetoes=vetoes)

    def set_recorder(self, every, burn_in=0, rung=None, keep_samples=True):
        """Recorder (include/ppde_hip.h, ppde_chains_set_recorder): the state after t completed iterations is recorded on the
        device when t > burn_in and (t - burn_in) % every == 0. rung None: every chain is a slot; rung r (tempering, set before):
        one slot per ensemble, the chain that holds rung r after that iteration's swap. keep_samples False: site counts only.
        every None clears it. Only before init()."""
        if every is None:
            self._call("set_recorder", None)
            self.recorder = None
            return
        cfg = _hip.RecordConfig(burn_in=int(burn_in), every=int(every), rung=-1 if rung is None else int(rung),
                                keep_samples=int(bool(keep_samples)))
        self._call("set_recorder", C.byref(cfg))
        self.recorder = dict(every=int(every), burn_in=int(burn_in), rung=None if rung is None else int(rung),
                             keep_samples=bool(keep_samples))

    def recorder_shape(self):
        """(rows recorded so far, row capacity, slots per row)."""
        d, cap, sl = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("recorder_shape", C.byref(d), C.byref(cap), C.byref(sl))
        return d.value, cap.value, sl.value

    def recorded(self, first=0, count=None):
        """What the recorder holds: rows [first, first + count) (default: all recorded so far) as idx uint8 [count, slots, L],
        energy / fitness fp32 [count, slots], chain int32 [count, slots] (local index of the chain that filled the slot) --
        None for a counts-only recorder --, site_counts uint64 [L, 20] over ALL rows recorded so far, and rows = that number."""
        done, _, slots = self.recorder_shape()
        first = int(first)
        count = done - first if count is None else int(count)
        L = self.model.L
        keep = self.recorder["keep_samples"]
        out = dict(idx=np.empty((max(count, 0), slots, L), np.uint8) if keep else None,
                   energy=np.empty((max(count, 0), slots), np.float32) if keep else None,
                   fitness=np.empty((max(count, 0), slots), np.float32) if keep else None,
                   chain=np.empty((max(count, 0), slots), np.int32) if keep else None,
                   site_counts=np.zeros((L, 20), np.uint64))
        self._call("recorder_read", first, count, *[_hip.ptr(out[k]) for k in ("idx", "energy", "fitness", "chain", "site_counts")])
        out["rows"] = done
        return out

    def set_pair_counts(self, sites=None):
        """Pair counts (include/ppde_hip.h, ppde_chains_set_pair_counts): letter co-occurrence counts over the recorder's rows and
        slots at `sites`, a strictly increasing list of 0-based residues (None: every residue). Needs a recorder; only before
        init()."""
        arr = None if sites is None else np.ascontiguousarray(np.asarray(sites, dtype=np.int32).reshape(-1))
        cfg = _hip.PairConfig(n_sites=0 if arr is None else int(arr.size),
                              sites=None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)))
        self._call("set_pair_counts", C.byref(cfg))

    def clear_pair_counts(self):
        self._call("set_pair_counts", None)

    def pair_counts(self):
        """(counts uint64 [S, 20, S, 20] over ALL rows recorded so far, sites int32 [S]): counts[i, a, j, b] = recorded (row, slot)
        pairs with letter a at residue sites[i] and letter b at residue sites[j]."""
        S = C.c_int32()
        self._call("pair_counts_shape", C.byref(S), None)
        sites = np.empty(S.value, np.int32)
        self._call("pair_counts_shape", None, _hip.ptr(sites))
        counts = np.zeros((S.value, 20, S.value, 20), np.uint64)
        self._call("pair_counts_read", _hip.ptr(counts))
        return counts, sites

    def set_archive(self, k):
        """Archive (include/ppde_hip.h, ppde_chains_set_archive): every chain keeps the k best distinct non-wild-type states it
        visited, 1 <= k <= 32. None clears it. Only before init()."""
        self._call("set_archive", None if k is None else C.byref(_hip.ArchiveConfig(k=int(k))))

    def archive(self):
        """What the archive holds: idx uint8 [n, K, L], energy / fitness fp32 [n, K], step int32 [n, K], count int32 [n]; every
        chain's entries by (energy descending, step ascending), the slots beyond count filled with 255, -inf, 0, -1."""
        K = C.c_int32()
        self._call("archive_shape", C.byref(K))
        n, k, L = self.n, K.value, self.model.L
        out = dict(idx=np.empty((n, k, L), np.uint8), energy=np.empty((n, k), np.float32), fitness=np.empty((n, k), np.float32),
                   step=np.empty((n, k), np.int32), count=np.empty(n, np.int32))
        self._call("archive_read", *[_hip.ptr(out[k_]) for k_ in ("idx", "energy", "fitness", "step", "count")])
        return out

    def set_stats(self, per_site=True):
        """Move statistics (include/ppde_hip.h, ppde_chains_set_stats): acceptances, jump distances, mutation counts and wild-type
        returns per (chain, rung), attempts and acceptances per (rung, path length) and, with per_site, changes per (rung,
        residue), counted on the device. None clears them. Only before init(), and after set_tempering() when there is a ladder."""
        self._call("set_stats", None if per_site is None else C.byref(_hip.StatsConfig(per_site=int(bool(per_site)))))

    def stats(self):
        """The counters so far, int64: iters, accepts, moved, jump_sum, dist_sum, wt_returns [n, R'], len_attempts, len_accepts
        [R', M], site_changes [R', L] (None when per_site is off); R' = max(rungs, 1), M = 2 pas_length - 1."""
        R, M, ps = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("stats_shape", C.byref(R), C.byref(M), C.byref(ps))
        out = {k: np.zeros((self.n, R.value), np.int64) for k in chain_stats.PER_CHAIN}
        out.update({k: np.zeros((R.value, M.value), np.int64) for k in chain_stats.PER_LENGTH})
        out["site_changes"] = np.zeros((R.value, self.model.L), np.int64) if ps.value else None
        self._call("stats_read", *[_hip.ptr(out[k]) for k in chain_stats.KEYS])
        return out

    def init(self, idx0):
        idx0 = idx0.to(self.model.device, torch.uint8).contiguous()
        if tuple(idx0.shape) != (self.n, self.model.L):
            raise ValueError(f"initial states must be [{self.n}, {self.model.L}] residue indices, got {tuple(idx0.shape)}")
        if int(idx0.max()) >= 20:
            raise ValueError("residue indices must be in 0..19")
        torch.cuda.current_stream(self.model.device).synchronize()
        self._call("init", _hip.ptr(idx0))
        self._initialised = True

    def run(self, steps, noise=None):
        """noise = (U int32 [steps,n], q fp32 [sum max_u, n, N], u fp32 [steps,n], max_u list) for rng_mode 0."""
        if noise is None:
            self._call("run", int(steps), None, None, None, None)
            return
        U, q, u, mus = noise
        dev = self.model.device
        U, q, u = (t.to(dev, non_blocking=False).contiguous() for t in (U, q, u))
        mu = np.ascontiguousarray(np.asarray(mus, dtype=np.int32))
        torch.cuda.current_stream(dev).synchronize()
        self._call("run", int(steps), _hip.ptr(U), _hip.ptr(q), _hip.ptr(u), _hip.ptr(mu))
        self._call("sync")   # the noise tensors must outlive the kernels

    def sync(self):
        self._call("sync")

    @property
    def steps_done(self):
        return self.lib.ppde_chains_steps_done(self.handle)

    def peek(self):
        n, L = self.n, self.model.L
        idx = np.empty((n, L), np.uint8)
        e, f = np.empty(n, np.float32), np.empty(n, np.float32)
        acc, dist = np.empty(n, np.uint8), np.empty(n, np.int32)
        self._call("peek", _hip.ptr(idx), _hip.ptr(e), _hip.ptr(f), _hip.ptr(acc), _hip.ptr(dist))
        return dict(idx=idx, energy=e, fitness=f, accepted=acc, dist=dist)

    def collect(self):
        n, L, rows = self.n, self.model.L, self.steps_done + 1
        out = dict(best_idx=np.empty((n, L), np.uint8), best_energy=np.empty(n, np.float32),
                   best_fitness=np.empty(n, np.float32), best_step=np.empty(n, np.int32),
                   energy_history=np.empty((rows, n), np.float32), fitness_history=np.empty((rows, n), np.float32),
                   random_traj=np.empty((rows, L), np.uint8) if self.cfg.random_chain >= 0 else None)
        self._call("collect", *[_hip.ptr(out[k]) for k in (
            "best_idx", "best_energy", "best_fitness", "best_step", "energy_history", "fitness_history", "random_traj")])
        return out

    def trace(self):
        t, n = self.steps_done, self.n
        out = dict(flat=np.empty((t, self.mu_max, n), np.int32), accepted=np.empty((t, n), np.uint8),
                   log_acc=np.empty((t, n), np.float32), U=np.empty((t, n), np.int32))
        self._call("trace", *[_hip.ptr(out[k]) for k in ("flat", "accepted", "log_acc", "U")])
        return out

    def graph_stats(self):
        """How the iterations so far were issued: graphs captured (all by init), captured inside a run (0), steps
        replayed from graphs / launched eagerly."""
        a, b, r, e = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._call("graph_stats", C.byref(a), C.byref(b), C.byref(r), C.byref(e))
        return dict(captures=a.value, captures_in_run=b.value, replayed_steps=r.value, eager_steps=e.value)

    def philox_dump(self, it, s):
        """What the device RNG draws for sub-step s of iteration it: (q [n, L + 20] Exp(1) race variates of the two-level draw --
        residue race [:, :L], letter race [:, L:] --, u [n] accept uniforms, U [n] path lengths)."""
        dev, n, L = self.model.device, self.n, self.model.L
        q = torch.empty(n, L * 20, device=dev)
        u = torch.empty(n, device=dev)
        U = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._call("philox_dump", int(it), int(s), _hip.ptr(q), _hip.ptr(u), _hip.ptr(U))
        return q[:, :L + 20].contiguous(), u, U

    def time_potts_in_situ(self, iters=200):
        """Potts kernel launches inside `iters` real iterations (Potts-only energy): (mean us from the predecessor kernel's end
        to the launch's end, launches timed, mean us of the dispatches' own start -> end stamps or None)."""
        v, k, d = C.c_float(), C.c_int(), C.c_float()
        self._call("time_potts_in_situ", int(iters), C.byref(v), C.byref(k), C.byref(d))
        return v.value, k.value, (d.value if d.value > 0 else None)

    def time_experts(self, reps=100):
        """Mean duration (us) of one evaluation of all experts of the energy (current states -> proposal slot)."""
        v = C.c_float()
        self._call("time_experts", int(reps), C.byref(v))
        return v.value

    def time_potts_kernel(self, reps=200):
        v = C.c_float()
        self._call("time_potts_kernel", int(reps), C.byref(v))
        return v.value


def gather_stats(shard, raw):
    """Chains.stats() of a sharded run: the per-chain arrays in global chain order, the others summed, so every rank ends with the
    full result."""
    out = {k: shard.gather(raw[k]) for k in chain_stats.PER_CHAIN}
    out.update({k: shard.sum(raw[k]) for k in chain_stats.PER_LENGTH + ("site_changes",)})
    return out


class PPDE_PAS(BaseSampler):
    _hinted = False

    def __init__(self, args):
        super().__init__()
        self.ppde_temp = 2  # locally balanced g(t) = sqrt(t)  (ppde.py:11)
        self.ppde_pas_length = args.ppde_pas_length
        self.nmut_threshold = args.nmut_threshold
        self.paper_results = args.paper_results
        self.rng = getattr(args, "ppde_rng", "torch")
        if self.rng not in ("torch", "philox"):
            raise ValueError("ppde_rng must be 'torch' or 'philox'")
        self.seed = getattr(args, "ppde_seed", None)
        if self.seed is None:
            self.seed = getattr(args, "seed", None)
        self.reuse_grad = getattr(args, "ppde_reuse_grad", True)
        self.use_graph = getattr(args, "ppde_use_graph", True)
        self.n_streams = getattr(args, "ppde_streams", 1)
        self.cpu_alias = getattr(args, "ppde_cpu_alias", False)
        self.shard = getattr(args, "ppde_shard", False)
        self.trace = getattr(args, "ppde_trace", False)
        self.library = getattr(args, "ppde_library", None)
        self.reversible = bool(getattr(args, "ppde_reversible", False))
        if self.reversible and self.paper_results:
            raise ValueError("ppde_reversible: paper_results restarts a rejected chain from its initial state, which is no "
                             "Metropolis step; the two cannot be combined")
        self.betas, self.swap_every = check_tempering(
            getattr(args, "ppde_betas", None), getattr(args, "ppde_swap_every", 1), self.reversible, self.n_streams)
        self.anneal_betas, self.anneal_every, self.deme = check_annealing(
            getattr(args, "ppde_anneal_betas", None), getattr(args, "ppde_anneal_every", 1) or 1, getattr(args, "ppde_deme", 0) or 0,
            self.reversible, self.betas, self.n_streams)
        self.anneal_adaptive = check_annealing_adaptive(
            getattr(args, "ppde_anneal_ess", None), getattr(args, "ppde_anneal_beta_start", None), getattr(args, "ppde_anneal_beta_end", 1.0),
            getattr(args, "ppde_anneal_min_step", None), getattr(args, "ppde_anneal_max_stages", None), self.anneal_every, self.deme,
            getattr(args, "ppde_anneal_betas", None), self.reversible, self.betas, self.n_streams)
        self.recombine_every, self.recombine_deme = check_recombination(
            getattr(args, "ppde_recombine_every", 0), getattr(args, "ppde_recombine_deme", 0), self.reversible, self.betas,
            self.anneal_betas if self.anneal_adaptive is None else self.anneal_adaptive, self.paper_results, self.n_streams)
        self.recombination = None
        self._recomb_logged = 0     # recombination events the periodic log has reported
        self._recomb_pairs = np.zeros(3, np.int64)   # so far: pairs with differ > 0, accepted ones of them, identical pairs
        self.sample_every, self.sample_burn_in, self.sample_rung, self.sample_counts_only, self.sample_pairs = check_recorder(
            getattr(args, "ppde_sample_every", 0), getattr(args, "ppde_sample_burn_in", 0), getattr(args, "ppde_sample_rung", None),
            getattr(args, "ppde_sample_counts_only", False), getattr(args, "ppde_sample_pairs", None), self.betas, self.n_streams)
        self.archive_k = check_archive(getattr(args, "ppde_archive", None), self.paper_results, self.n_streams)
        self.forbid, self.forbid_allow_native = check_forbid(getattr(args, "ppde_forbid", None), getattr(args, "ppde_forbid_strict", False),
                                                             self.reversible, self.paper_results)
        self.forbidden = None
        self.stats_spec = check_stats(getattr(args, "ppde_stats", None), self.n_streams)
        self.tempering = self.annealing = self.samples = self.archive = self.stats = None     # what the last run() collected
        self.noise_bytes = getattr(args, "ppde_noise_bytes", 96 << 20)   # host->device noise is uploaded in chunks of about this size
        self.last_chains = None
        self._anneal_logged = 0     # annealing events the periodic log of the running run() has reported
        self.timings = {}       # seconds of the last run(): setup (chains + hipGraph capture), iterations, log path, collect

    def approximate_energy_change(self, score_change):
        return score_change / self.ppde_temp

    def _plan(self, initial_population, num_steps, min_pos, max_pos):
        """Everything of a run that is decided on the host, and every refusal that needs no device: the library's words of a
        reversible run (None otherwise), rungs R and deme D (0: off), the pair sites, the recorded chain and this rank's Shard."""
        n_global, L = int(initial_population.size(0)), int(initial_population.size(1))
        lib_words = None
        if self.reversible:
            # a reversible run always has a library, the range folded in: the restriction is hard and the law exact. The
            # population is checked on the host, before anything touches the device.
            lib = design_library.full_library(L) if self.library is None else design_library.as_words(self.library, L)
            lib_words = design_library.fold_range(lib, min_pos, max_pos)
            design_library.check_population(lib_words, initial_population.detach().argmax(-1).cpu().numpy())
        if self.forbid is not None:
            check_forbid_population(self.forbid, self.forbid_allow_native, self._wt_idx,
                                    initial_population.detach().argmax(-1).cpu().numpy())
        R = 0 if self.betas is None else int(self.betas.size)
        if R and n_global % R:
            raise ValueError(f"ppde_betas: the population of {n_global} chains is no multiple of the {R} rungs of the ladder")
        if self.sample_every and recorder_rows(int(num_steps), self.sample_burn_in, self.sample_every) == 0:
            raise ValueError(f"ppde_sample_every: no iteration of {int(num_steps)} would be recorded (burn-in {self.sample_burn_in}, "
                             f"every {self.sample_every})")
        pair_sites = None
        if self.sample_pairs is not None:               # (host only: the library's words as the chains will get them)
            words = lib_words
            if words is None and self.library is not None:
                words = design_library.fold_range(design_library.as_words(self.library, L), min_pos, max_pos)
            pair_sites = pair_sites_of(self.sample_pairs, L, min_pos, max_pos, words)
            if pair_sites is not None and pair_sites.size == 0:
                raise ValueError("ppde_sample_pairs: the selection holds no residue")
        random_idx = np.random.randint(0, n_global)                       # ppde.py:37 (same numpy RNG consumption)
        rank, ws = world() if self.shard else (0, 1)
        # (comm: ws > 1, or the one-rank rehearsal of the RCCL path; never in a run that does not shard)
        shard = Shard(n_global, rank, ws, comm=self.shard and collectives_active())
        cut = boundary_cut(shard.starts, R) if R else None
        if cut:
            raise ValueError(f"ppde_betas: the shard boundary at chain {cut[1]} (rank {cut[0]} of {ws}) cuts an ensemble of {R} chains")
        D = 0
        if self.anneal_betas is not None:
            D = check_demes(n_global, self.deme, num_steps, self.anneal_every, self.anneal_betas.size - 1, shard.starts)
        elif self.anneal_adaptive is not None:
            D = check_demes(n_global, self.deme, num_steps, self.anneal_every, self.anneal_adaptive["max_stages"], shard.starts)
        X = 0
        if self.recombine_every:
            X = check_recombination_demes(n_global, self.recombine_deme, num_steps, self.recombine_every, shard.starts)
        return SimpleNamespace(L=L, lib_words=lib_words, R=R, D=D, X=X, pair_sites=pair_sites, random_idx=random_idx, shard=shard)

    def _configured_chains(self, model, which, plan, num_steps, min_pos, max_pos, random_idx, seed):
        """This rank's Chains with every mode of the run set, before init()."""
        shard, lib_words = plan.shard, plan.lib_words
        if self.library is not None and not self.reversible:
            # the range goes INTO the library (exact) and the chains run over the full range: no entry of a library run is
            # masked by the leaky range mask. The same words on every rank.
            lib_words = design_library.fold_range(design_library.as_words(self.library, plan.L), min_pos, max_pos)
        chains = Chains(model, shard.n, num_steps, self.ppde_pas_length, self.nmut_threshold, self.paper_results,
                        0 if lib_words is not None else min_pos, plan.L - 1 if lib_words is not None else max_pos, which,
                        0 if self.rng == "torch" else 1, self.reuse_grad, self.cpu_alias, self.trace,
                        random_idx - shard.lo if shard.lo <= random_idx < shard.hi else -1, self.use_graph, seed, shard.lo,
                        self.n_streams)
        self.last_chains = chains
        if lib_words is not None:
            chains.set_library(lib_words)
        if self.reversible:
            chains.set_reversible(True)
        if self.forbid is not None:
            chains.set_forbidden(self.forbid, self.forbid_allow_native)
        if plan.R:
            chains.set_tempering(self.betas, self.swap_every)
        if plan.D and self.anneal_adaptive is not None:
            ad = self.anneal_adaptive
            chains.set_annealing_adaptive(ad["beta_start"], ad["beta_end"], ad["ess_target"], self.anneal_every, plan.D, ad["max_stages"],
                                          ad["min_step"])
        elif plan.D:
            chains.set_annealing(self.anneal_betas, self.anneal_every, plan.D)
        if plan.X:
            chains.set_recombination(self.recombine_every, plan.X)
        if self.sample_every:
            chains.set_recorder(self.sample_every, self.sample_burn_in, self.sample_rung, not self.sample_counts_only)
        if self.sample_pairs is not None:
            chains.set_pair_counts(plan.pair_sites)
        if self.archive_k:
            chains.set_archive(self.archive_k)
        if self.stats_spec is not None:
            chains.set_stats(self.stats_spec is True)
        return chains

    def _advance(self, chains, shard, steps, N):
        """`steps` iterations; in replay mode the host's noise goes up in chunks of about noise_bytes."""
        if self.rng != "torch":
            chains.run(steps)
            return
        kmax = max(1, int(self.noise_bytes // (self.ppde_pas_length * 2 * shard.n * N * 4 + 1)))
        while steps > 0:
            k = min(kmax, steps)
            chains.run(k, draw_chunk(k, shard.n_global, N, self.ppde_pas_length, rows=(shard.lo, shard.hi)))
            steps -= k

    def _log(self, i, chains, plan, model, oracle, first=False):
        shard = plan.shard
        pk = chains.peek()
        # (the one-hot form the oracle takes is expanded on the device: n x L bytes cross PCIe instead of n x L x 20 floats)
        x_now = model.idx_to_onehot(torch.from_numpy(np.ascontiguousarray(shard.gather(pk["idx"]))))
        gt = oracle(x_now).detach().cpu().numpy()
        # (one call for the three rows: np.quantile's fixed cost is ~60 us, a seventh of a log line)
        fq, gq, eq = np.quantile(np.stack([shard.gather(pk["fitness"]), gt, shard.gather(pk["energy"])]), [0.5, 0.9], axis=1).T
        print(f'[Iteration {i}] energy: 50% {eq[0]:.3f}, 90% {eq[1]:.3f}', flush=not first)
        if first:
            print(f'[Iteration {i}] pred fit 50% {fq[0]:.3f}, 90% {fq[1]:.3f}')
            print(f'[Iteration {i}] oracle fit 50% {gq[0]:.3f}, 90% {gq[1]:.3f}')
            print('')
        else:
            print(f'[Iteration {i}] pred 50% {fq[0]:.3f}, 90% {fq[1]:.3f}', flush=True)
            print(f'[Iteration {i}] oracle 50% {gq[0]:.3f}, 90% {gq[1]:.3f}', flush=True)
            print(f'   # accepted = {float(shard.gather(pk["accepted"]).sum())}')
            print(f'   # dist = {float(shard.gather(pk["dist"]).astype(np.float32).mean())}')
            self._log_modes(chains, plan)
            print('', flush=True)

    def _log_modes(self, chains, plan):
        """The lines the optional modes add to a periodic log: swaps, the annealing stage, the move statistics."""
        shard, R, D = plan.shard, plan.R, plan.D
        if R:
            ts = self._swap_counts(chains, shard, R)
            print(f'   # swaps accepted = {int(ts["swap_accepts"].sum())} / {int(ts["swap_attempts"].sum())}')
        if D:
            self._log_annealing(chains, shard, D)
        if plan.X:
            self._log_recombination(chains, shard)
        if self.forbid is not None:
            v = shard.gather(chains.forbidden_state()["vetoes"])
            print("   " + chain_motifs.log_line(chain_motifs.summarise(v, chains.steps_done, self.forbid.text)))
        if self.stats_spec is not None:
            print(chain_stats.log_line(gather_stats(shard, chains.stats())))

    def _log_annealing(self, chains, shard, D):
        """One line when events happened since the last log: the latest stage, its beta, the smallest ESS and the slots replaced."""
        _, _, ev = chains.annealing_shape()
        if ev > self._anneal_logged:
            st = chains.annealing_state(self._anneal_logged, ev - self._anneal_logged)
            ess = shard.gather(st["ess"], dim=1, size=D)
            replaced = sum(int((row != np.arange(shard.n)).sum()) for row in st["parent"])
            replaced = int(shard.sum(np.array([replaced], np.int64))[0])
            if self.anneal_adaptive is not None:         # every deme at its own beta: their spread and how many have arrived
                b = shard.gather(st["beta_after"], dim=1, size=D)[-1]
                print(f'   # annealing: stage {ev}, beta min / median / max = {float(b.min()):.6g} / {float(np.median(b)):.6g} / '
                      f'{float(b.max()):.6g}, arrived = {int((b >= np.float32(self.anneal_adaptive["beta_end"])).sum())} of {b.size} '
                      f'demes, min ESS = {float(ess.min()):.2f} of {D}, slots replaced = {replaced}')
                self._anneal_logged = ev
                return
            print(f'   # annealing: stage {ev} of {self.anneal_betas.size - 1}, beta = {float(self.anneal_betas[ev]):.6g}, '
                  f'min ESS = {float(ess.min()):.2f} of {D}, slots replaced = {replaced}')
            self._anneal_logged = ev

    def _log_recombination(self, chains, shard):
        """One line when events happened since the last log: acceptance so far over the pairs with differ > 0, and the share of
        identical pairs."""
        ev = chains.recombination_shape()[3]
        if ev > self._recomb_logged:
            st = chains.recombination_state(self._recomb_logged, ev - self._recomb_logged)
            first = np.arange(shard.n)[None] < st["partner"]
            real = first & (st["differ"] > 0)
            new = np.array([real.sum(), (real & (st["outcome"] == 1)).sum(), (first & (st["differ"] == 0)).sum()], np.int64)
            self._recomb_pairs = self._recomb_pairs + shard.sum(new)
            real_n, acc_n, same_n = (int(v) for v in self._recomb_pairs)
            print(f'   # recombination: event {ev}, accepted {acc_n} / {real_n} of the pairs that differ'
                  f'{f" ({acc_n / real_n:.3f})" if real_n else ""}, identical pairs {same_n / max(real_n + same_n, 1):.3f}')
            self._recomb_logged = ev

    def _collect_recombination(self, chains, shard, X):
        """Per-chain rows [events, n_global] in global chain order, partners as GLOBAL indices; cut [events, n, 2]; the summary."""
        if not X:
            return None
        st = chains.recombination_state()
        st["partner"] = shard.to_global(st["partner"])
        rc = {k: shard.gather(st[k], dim=1) for k, _ in Chains.RECOMBINATION_FIELDS}
        rc.update(deme=X, every=self.recombine_every, open_sites=st["open_sites"], events=st["events"],
                  cut=np.stack([rc["lo"], rc["hi"]], -1))
        rc["summary"] = chain_recombine.summarise(rc)
        return rc

    @staticmethod
    def _swap_counts(chains, shard, R):
        """swap_accepts / swap_attempts [n_global / R, R - 1] (a ladder of one rung has no pairs: nothing to gather)."""
        ts = chains.tempering_state()
        return {k: shard.gather(ts[k], size=R) if R > 1 else ts[k] for k in ("swap_accepts", "swap_attempts")}

    def _collect_tempering(self, chains, shard, R):
        if not R:
            return None
        ts = self._swap_counts(chains, shard, R)
        return dict(betas=self.betas.copy(), rung_history=shard.gather(chains.tempering_history(), dim=1),
                    swap_attempts=ts["swap_attempts"], swap_accepts=ts["swap_accepts"])

    def _collect_annealing(self, chains, shard, D):
        if not D:
            return None
        st = chains.annealing_state()
        ad = self.anneal_adaptive
        betas = self.anneal_betas.copy() if ad is None else np.array([ad["beta_start"], ad["beta_end"]], np.float32)
        an = dict(betas=betas, deme=D, every=self.anneal_every,
                  parent=shard.gather(shard.to_global(st["parent"]), dim=1), pre_energy=shard.gather(st["pre_energy"], dim=1),
                  log_mean_w=shard.gather(st["log_mean_w"], dim=1, size=D), ess=shard.gather(st["ess"], dim=1, size=D),
                  beta_now=shard.gather(st["beta"]))
        if ad is None:
            an["summary"] = chain_anneal.summarise(an["parent"], an["log_mean_w"], an["ess"], an["betas"])
            return an
        after = shard.gather(st["beta_after"], dim=1, size=D)
        an.update(ess_target=ad["ess_target"], min_step=ad["min_step"], max_stages=ad["max_stages"],
                  beta_path=np.concatenate([np.full((1, after.shape[1]), betas[0], np.float32), after], 0))
        an["summary"] = chain_anneal.summarise(an["parent"], an["log_mean_w"], an["ess"], an["beta_path"], beta_end=betas[1])
        return an

    def _collect_samples(self, chains, shard, R):
        if not self.sample_every:
            return None
        rec = chains.recorded()
        out = dict(rows=rec["rows"], site_counts=shard.sum(rec["site_counts"]), idx=None, energy=None, fitness=None, chain=None,
                   pair_counts=None, pair_sites=None)
        if self.sample_pairs is not None:
            pc, ps = chains.pair_counts()
            out.update(pair_counts=shard.sum(pc), pair_sites=ps)
        if not self.sample_counts_only:
            rec["chain"] = shard.to_global(rec["chain"])
            # (one slot per ensemble with a ladder, per chain without: shard boundaries are multiples of R, equal slot blocks)
            out.update({k: shard.gather(rec[k], dim=1, size=R or 1) for k in ("idx", "energy", "fitness", "chain")})
        return out

    def _collect_archive(self, chains, shard):
        if not self.archive_k:
            return None
        arc = {k: shard.gather(v) for k, v in chains.archive().items()}      # (global chain order)
        arc["chain"] = np.arange(shard.n_global, dtype=np.int64)
        arc["candidates"] = chain_archive.merge(arc["idx"], arc["energy"], arc["fitness"], arc["step"], arc["count"])
        return arc

    def _collect_forbidden(self, chains, shard):
        if self.forbid is None:
            return None
        st = chains.forbidden_state()
        v = shard.gather(st["vetoes"])
        return dict(text=st["text"], allow_native=st["allow_native"], active=st["active"], vetoes=v,
                    summary=chain_motifs.summarise(v, chains.steps_done, st["text"]))

    def _collect_stats(self, chains, shard):
        if self.stats_spec is None:
            return None
        st = gather_stats(shard, chains.stats())
        st["chain"] = np.arange(shard.n_global, dtype=np.int64)
        st["betas"] = None if self.betas is None else self.betas.copy()
        st["summary"] = chain_stats.summarise(st, st["betas"])
        return st

    def run(self, initial_population, num_steps, energy_function, min_pos, max_pos, oracle, log_every=50):
        print(min_pos, max_pos)
        model = getattr(energy_function, "model", None)
        if model is None or not hasattr(energy_function, "which"):
            raise TypeError("PPDE_PAS.run needs a ppde_amd energy function (ProteinProductOfExperts / ProteinSupervised); "
                            "there is no generic torch fallback")
        min_pos, max_pos = int(min_pos), int(max_pos)
        # ---- host-only plan: every refusal that needs no device comes from here
        self._wt_idx = np.asarray(model.wt_idx) if self.forbid is not None else None
        plan = self._plan(initial_population, num_steps, min_pos, max_pos)
        shard, R, D, L, random_idx = plan.shard, plan.R, plan.D, plan.L, plan.random_idx
        idx0 = model.onehot_to_idx(initial_population)
        # ---- RNG agreement
        # (63 bits whatever the rank count: the key travels through an int64 tensor when ranks agree on it, and a run's
        # Philox streams must not depend on how many ranks there are)
        seed = (self.seed if self.seed is not None else torch.initial_seed()) & (2 ** 63 - 1)
        if shard.comm:  # one recorded chain and one Philox key for the whole job, whatever each rank's host RNG state is
            random_idx, seed = agree_from_rank0([random_idx, seed])
        if self.rng == "torch" and not PPDE_PAS._hinted:
            PPDE_PAS._hinted = True
            print("[ppde_amd] ppde_rng='torch' replays the reference's random stream: every iteration waits for torch's CPU exponential_ "
                  "(~100 iterations/s at 128 chains). --ppde_rng philox draws on the device: hundreds of times faster, same law, "
                  "another trajectory.", file=sys.stderr, flush=True)
        # ---- chains
        t_begin = time.perf_counter()
        t_log = 0.0
        chains = self._configured_chains(model, energy_function.which, plan, num_steps, min_pos, max_pos, random_idx, seed)
        chains.init(idx0[shard.lo:shard.hi])
        self._anneal_logged = self._recomb_logged = 0
        self._recomb_pairs = np.zeros(3, np.int64)
        chains.sync()
        t_setup = time.perf_counter() - t_begin
        # ---- iterations, with the log
        t0 = time.perf_counter()
        self._log(0, chains, plan, model, oracle, first=True)
        t_run0 = time.perf_counter()
        t_log0 = t_run0 - t0
        done = 0
        while done < num_steps:
            # next iteration index i with i > 0 and (i+1) % log_every == 0  ->  stop after i+1 steps
            stop = min(num_steps, ((done // log_every) + 1) * log_every) if log_every > 0 else num_steps
            self._advance(chains, shard, stop - done, L * 20)
            done = stop
            i = done - 1
            if log_every > 0 and i > 0 and (i + 1) % log_every == 0:
                chains.sync()
                t0 = time.perf_counter()
                self._log(i, chains, plan, model, oracle)
                t_log += time.perf_counter() - t0
        chains.sync()
        t_run = time.perf_counter() - t_run0 - t_log
        # ---- collect
        t0 = time.perf_counter()
        res = chains.collect()
        best_x = torch.from_numpy(idx_to_onehot(shard.gather(res["best_idx"]))).float().to(initial_population.device)
        e_hist, f_hist = shard.gather(res["energy_history"], dim=1), shard.gather(res["fitness_history"], dim=1)
        # (only its owner recorded the random chain; the other ranks of a sharded run hand in a blank)
        rtraj = res["random_traj"] if res["random_traj"] is not None else np.zeros((num_steps + 1, L), np.uint8)
        rtraj = shard.broadcast(rtraj, shard.owner(random_idx))
        random_traj = list(idx_to_onehot(rtraj, dtype=np.float32))     # T + 1 arrays [L, 20] (views of one expansion)
        best_e, best_f = shard.gather(res["best_energy"]), shard.gather(res["best_fitness"])
        self.tempering = self._collect_tempering(chains, shard, R)
        self.annealing = self._collect_annealing(chains, shard, D)
        self.recombination = self._collect_recombination(chains, shard, plan.X)
        self.samples = self._collect_samples(chains, shard, R)
        self.archive = self._collect_archive(chains, shard)
        self.stats = self._collect_stats(chains, shard)
        self.forbidden = self._collect_forbidden(chains, shard)
        if shard.n_global == 1:
            # the reference's single-chain shapes (ppde.py:178-183; the ensemble's `.squeeze()`, nets.py:442, makes one chain's
            # fitness a scalar): fitness_history (T+1,) next to energy_history (T+1, 1); with ProteinSupervised the energy IS
            # that scalar, so energy_history is (T+1,) too and best_energy / best_fitness are 0-dim
            f_hist = f_hist.reshape(-1)
            if (energy_function.which & 7) == 2:
                e_hist, best_e, best_f = e_hist.reshape(-1), best_e.reshape(()), best_f.reshape(())
        # (log_first_s: the line of iteration 0, which in a fresh process carries the first use of the oracle's torch kernels)
        self.timings = {"setup_s": t_setup, "iterations_s": t_run, "log_s": t_log0 + t_log, "log_first_s": t_log0,
                        "log_calls": 1 + (num_steps // log_every if log_every > 0 else 0),
                        "collect_s": time.perf_counter() - t0, "graph": chains.graph_stats()}
        return (best_x, best_e, best_f, e_hist, f_hist, random_traj)

"""Host side of population annealing (include/ppde_hip.h, ppde_chains_set_annealing): what the recorded events say, in plain numpy.

The raw arrays, as `Chains.annealing_state()` / `PPDE_PAS.annealing` hold them: parent int [events, n] (index of the ancestor of
every slot, in the same numbering as the slots: local for one object, global for a gathered run; the identity where nothing was
replaced), log_mean_w and ess float64 [events, n / D], betas fp32 [S + 1] -- or, of an adaptive run
(ppde_chains_set_annealing_adaptive), the path fp32 [events + 1, n / D] each deme chose: row 0 beta_start, row k + 1 beta_after of
event k."""
import numpy as np


def compose(parent):
    """founder int64 [events + 1, n]: the slot of the START population each slot descends from after 0, 1, ... events (row 0 the
    identity; row k + 1 = row k read at the parents of event k)."""
    parent = np.asarray(parent, np.int64)
    n = parent.shape[1]
    out = np.empty((parent.shape[0] + 1, n), np.int64)
    out[0] = np.arange(n)
    for k in range(parent.shape[0]):
        out[k + 1] = out[k][parent[k]]
    return out


def summarise(parent, log_mean_w, ess, betas, beta_end=None):
    """What a run's events say (events = rows recorded, possibly fewer than the schedule's stages):
        deme                    D = n / demes
        log_z_ratio             [demes]   sum over the events of log_mean_w: each deme's estimate of log(Z_beta[events] / Z_beta[0])
        log_z_ratio_mean, log_z_ratio_std   mean and spread (sample standard deviation; nan with one deme) over the demes
        ess                     [events, demes] as given;  ess_min, ess_mean [events] over the demes
        replaced                [events]  slots that took another chain's state
        founders_alive          [events, demes]  founders of each deme that still have descendants after each event
        betas                   [events + 1] the inverse temperatures passed so far
    With a 2-D path `betas` [events + 1, demes] of an adaptive run (beta_end: where it leads; default the path's largest entry):
        betas                   [events + 1, demes] as given
        arrived                 [demes] bool: the deme holds beta_end
        stages                  [demes] the events each deme took until beta_end, or -1
        log_z_ratio_mean, log_z_ratio_std   over the ARRIVED demes only (nan without one, std nan below two): the ratios of demes
                                at different beta estimate different quantities and are not comparable"""
    parent = np.asarray(parent, np.int64)
    lmw, ess = np.asarray(log_mean_w, np.float64), np.asarray(ess, np.float64)
    events, n = parent.shape
    demes = lmw.shape[1] if lmw.ndim == 2 and lmw.shape[1] else 1
    D = n // demes
    if (parent // D != (np.arange(n) // D)[None]).any():
        raise ValueError("an ancestor lies outside its slot's deme")
    founder = compose(parent)
    alive = np.array([[np.unique(founder[k + 1, d * D:(d + 1) * D]).size for d in range(demes)] for k in range(events)],
                     np.int64).reshape(events, demes)
    lz = lmw.sum(0) if events else np.zeros(demes)
    betas = np.asarray(betas, np.float32)
    if betas.ndim == 2:
        path = betas[:events + 1].copy()
        if path.shape[1] != demes:
            raise ValueError(f"the beta path has {path.shape[1]} columns for {demes} demes")
        end = np.float32(path.max() if beta_end is None else beta_end)
        at_end = path >= end
        arrived = at_end[-1]
        stages = np.where(arrived, at_end.argmax(0), -1).astype(np.int64)
        got = lz[arrived]
        return dict(deme=D, log_z_ratio=lz, log_z_ratio_mean=float(got.mean()) if got.size else float("nan"),
                    log_z_ratio_std=float(got.std(ddof=1)) if got.size > 1 else float("nan"),
                    ess=ess, ess_min=ess.min(1) if events else np.zeros(0), ess_mean=ess.mean(1) if events else np.zeros(0),
                    replaced=(parent != np.arange(n)[None]).sum(1), founders_alive=alive, betas=path, arrived=arrived, stages=stages)
    return dict(deme=D, log_z_ratio=lz, log_z_ratio_mean=float(lz.mean()),
                log_z_ratio_std=float(lz.std(ddof=1)) if demes > 1 else float("nan"),
                ess=ess, ess_min=ess.min(1) if events else np.zeros(0), ess_mean=ess.mean(1) if events else np.zeros(0),
                replaced=(parent != np.arange(n)[None]).sum(1), founders_alive=alive,
                betas=np.asarray(betas, np.float32)[:events + 1].copy())

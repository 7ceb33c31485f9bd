"""Helpers of the chain kernels' dynamic-range tests (tests/test_chain_range_cpu.py, tests/test_chain_range_gpu.py).

The device-RNG chain kernels (ppde_amd/csrc/pas.h: propose_body_dev, reverse_rows_dev) take exp(z - mref) against a FIXED softmax
reference per launch, mref = min(beta * spread / 2, 64), spread = max - min of the staged gradient row (over the proposal range for
the forward rows, over every residue for the reverse rows). They are the only kernels of the project whose correctness depends on
the MAGNITUDE of their input. What is here:

  spread_model / capped_model   Potts-only models (which = 1) on synthetic.make_potts with planted fields, so that the oracle's
                                gradient has a chosen spread, or a capped chain's revert logits lie a chosen depth below mref;
  CELLS                         the matrix both modules walk (the CPU module classifies every cell, the GPU module runs it);
  score / score64               the accept log-ratio of a RECORDED path (draws, path lengths, accept bits given) through the
                                reference's own iteration functions (orc.pas_iteration under helpers_library.masked_oracle,
                                helpers_reversible.reversible_iteration, helpers_tempering.ScaledEnergy) on fp32 or .double() inputs;
  fixed_reference_fp32          the device's row arithmetic restated in numpy float32 (fixed reference, summation trees, c = 1 / S1,
                                the v_med3 clamp, library zeroing, residue masses, S3, the guard on S1), and
  emulated(...)                 the context in which the reference's iteration functions form their rows with it -- the second
                                yardstick evaluation, the classifier of every sub-step's S1, and the place the faults are planted."""
import contextlib
import math

import numpy as np
import torch

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht
import ppde_oracle as orc
from ppde_amd import library as dl
from ppde_amd import synthetic

A = 20
EPS = np.float32(2.0 ** -23)
ONE_M = np.float32(1.0) - EPS
MREF_CAP = 64.0
S1_MIN = np.float32(2.0 ** -125)              # pas.h PAS_S1_MIN: a normaliser below it (or non-finite) is flagged PPDE_ERR_NUMERIC
N, T, PAS = 32, 12, 3
SIZES = {24: (4, 16), 104: (23, 76), 237: (0, 237)}        # L -> Potts window (start, length) = the proposal range: 1, 2, 3 groups per thread
GAP_TOL, ACC_TOL = 1e-5, 2e-4                 # the project's near-tie thresholds (helpers_modes)
LADDER_HOT, LADDER_CONTROL = (2.0, 1.0, 0.5, 0.25), (1.0, 0.5, 0.25, 0.125)
CLASSES = ("normal", "denormal", "recip_inf", "zero", "inf")


class NumericFlag(ValueError):
    """What the emulation raises where the device flags PPDE_ERR_NUMERIC (a forward row without mass)."""


# ------------------------------------------------------------------------------------------------ models
def _energy(J, h, i0, wt):
    return orc.EnergyOracle(orc.PottsOracle(J, h, i0, torch.as_tensor(np.asarray(wt).astype(np.int64))), None, 0.0)


def _grad(J, h, i0, state):
    x = torch.as_tensor(np.asarray(state).astype(np.int64)).reshape(1, -1)
    return _energy(J, h, i0, state).energy_grad(x)[2][0].numpy()


def spread_of(g, lo, hi):
    g = np.asarray(g)[..., lo:hi + 1, :]
    return float(g.max() - g.min())


def spread_model(L, win, D, kind, seed=3):
    """The wild type, J and h of synthetic.make_potts(win[1], seed) (tests/helpers_modes.toy_parts' recipe) with two planted fields
    so that the oracle's gradient AT THE WILD TYPE has spread D over the proposal range win[0] .. win[0] + win[1] - 1:
      within  g[l0][k0] = +D/2 and g[l0][wt[l0]] = -D/2: one residue carries the spread, its logits reach D/2 (the overflow side);
      across  g[l0][k0] = +D/4 and g[l1][k1] = -3D/4, k1 != wt[l1]: mref follows D, no logit goes beyond D/8 (the underflow side);
      D = "tiny": J and h scaled by 2^-14, nothing planted (logits ~1e-4, a near-uniform proposal).
    Returns dict(L, win, lo, hi, wt, J, h, i0, kind, spread = the REALISED spread the fp32 oracle sees, sites)."""
    lo, Lp = win
    wt = np.random.default_rng(seed).integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(Lp, seed=seed)
    i_a, i_b = 3, 9                                                        # window coordinates of the planted residues
    l0, l1 = lo + i_a, lo + i_b
    k0, k1 = (int(wt[l0]) + 7) % A, (int(wt[l1]) + 5) % A
    if D == "tiny":
        J, h = J * np.float32(2.0 ** -14), h * np.float32(2.0 ** -14)
    else:
        g0 = _grad(J, h, lo, wt)
        h = h.copy()
        if kind == "within":
            h[i_a, k0] += np.float32(D / 2.0 - g0[l0, k0])
            h[i_a, int(wt[l0])] -= np.float32(D / 2.0 + g0[l0, int(wt[l0])])
        elif kind == "across":
            h[i_a, k0] += np.float32(D / 4.0 - g0[l0, k0])
            h[i_b, k1] -= np.float32(3.0 * D / 4.0 + g0[l1, k1])
        else:
            raise ValueError(kind)
    out = dict(L=L, win=win, lo=lo, hi=lo + Lp - 1, wt=wt, J=J, h=h, i0=lo, kind=kind, sites=((l0, k0), (l1, k1)), x0=None,
               nmut=0, lib=None)
    out["spread"] = spread_of(_grad(J, h, lo, wt), out["lo"], out["hi"])
    return out


def capped_start(wt, sites, letters):
    """The wild type with `letters` at `sites`: run with nmut_threshold = len(sites) the chain sits at the mutation cap from
    iteration 0, where only the reverts of these sites are admissible."""
    x = np.asarray(wt).copy()
    for s, k in zip(sites, letters):
        assert int(k) != int(wt[s])
        x[s] = k
    return x


def capped_model(depth, gap=5.0, base=280.0, L=24, seed=3, beta=1.0):
    """spread_model(L, across, base) with a start state of two mutations (residues lo + 5 and lo + 11) whose fields are set so that,
    in the row of the START state, the two revert logits are beta * z0 and beta * (z0 - gap) with beta * z0 - mref = depth, mref =
    min(beta * base / 2, 64). Each revert's gradient difference is planted three quarters on the wild-type letter, one on the mutated one, and
    must stay inside the base spread (asserted), so that mref is the base's. Returns the model with x0, cap_sites, cap_letters, spread
    and depth = the REALISED figures from the fp32 oracle's gradient at x0."""
    m = spread_model(L, SIZES[L], base, "across", seed)
    lo, wt = m["lo"], m["wt"]
    s = (lo + 5, lo + 11)
    letters = [(int(wt[p]) + 3) % A for p in s]
    x0 = capped_start(wt, s, letters)
    h = m["h"].copy()
    g = _grad(m["J"], h, lo, x0)
    z0 = (depth + min(beta * base / 2.0, MREF_CAP)) / beta
    for i, (p, k) in enumerate(zip(s, letters)):
        zi = z0 - gap * i                                                  # (g[wt] - g[mutated letter]) / 2 = the revert's logit
        assert -base / 2.0 <= zi <= base / 6.0, "the planted revert would widen the spread"
        h[p - lo, int(wt[p])] += np.float32(1.5 * zi - g[p, int(wt[p])])     # the base spread runs from -3/4 base to +1/4 base
        h[p - lo, k] += np.float32(-0.5 * zi - g[p, k])
    m.update(h=h, x0=x0, cap_sites=s, cap_letters=letters)
    g = _grad(m["J"], h, lo, x0)
    m["spread"] = spread_of(g, m["lo"], m["hi"])
    z = [np.float32(beta) * ((g[p, int(wt[p])] - g[p, k]) * np.float32(0.5)) for p, k in zip(s, letters)]
    m["depth"] = float(max(z) - min(beta * m["spread"] / 2.0, MREF_CAP))
    m["revert_gap"] = float(z[0] - z[1])
    return m


def _couple(J, i, k, j, l, c):
    """J with the coupling between (window residue i, letter k) and (j, l) raised by c, kept symmetric: g[j][l] gains c while the
    chain holds k at i (and the other way round), the energy gains c while it holds both."""
    J[i, j, k, l] += np.float32(c)
    J[j, i, l, k] += np.float32(c)


def gy_overflow_model(c=330.0, L=24, seed=3):
    """A model whose large spread appears only in g_y: spread_model(across, 40) with the move (la, ka) made dominant (its gradient
    entry at 30) and coupled by `c` to (lb, kb). At the wild type nothing of the coupling shows; once a path has moved la to ka,
    g_y[lb][kb] = c and the default-mode reverse rows (no masks, every residue) hold a logit of c / 2 against mref = 64."""
    m = spread_model(L, SIZES[L], 40, "across", seed)
    lo, wt = m["lo"], m["wt"]
    ia, ib = 6, 13
    ka, kb = (int(wt[lo + ia]) + 9) % A, (int(wt[lo + ib]) + 11) % A
    h, J = m["h"].copy(), m["J"].copy()
    h[ia, ka] += np.float32(30.0 - _grad(J, h, lo, wt)[lo + ia, ka])
    _couple(J, ia, ka, ib, kb, c)
    y = wt.copy(); y[lo + ia] = ka
    gy = _grad(J, h, lo, y)
    m.update(h=h, J=J, gy_move=(lo + ia) * A + ka, spread=spread_of(_grad(J, h, lo, wt), m["lo"], m["hi"]), spread_y=spread_of(gy, 0, L - 1),
             top_y=float((gy[lo + ib, kb] - gy[lo + ib, int(wt[lo + ib])]) * 0.5 - MREF_CAP))
    return m


def capped_reverse_model(depth, gap=5.0, L=24, seed=3):
    """Capped REVERSE rows of reversible mode (nmut_threshold 2): the start state x0 holds one mutation (s0 -> m0). Couplings of the
    letter ka at residue la with (s0, wild type) [c2], (s0, m0) [c2 + c3] and (lb, kb) [-200] make the path  la -> ka, s0 -> wild type
    the dominant one (x0 -> x1, capped -> y) and show in g_y only: the reverse row of its first sub-step is row(g_y, x1), whose only
    admissible entries are the two reverts, at depth (revert of la) and depth - gap (revert of s0) below mref_y = 64 (g_y's spread
    is beyond 200 through (lb, kb); g_x0 has none of it but the forward logit (c2 + c3) / 2 of la -> ka).
    Returns the model with x0, depth = the REALISED depth of that row from the fp32 oracle's g_y."""
    m = spread_model(L, SIZES[L], 40, "across", seed)
    lo, wt = m["lo"], m["wt"]
    i_s, ia, ib = 5, 7, 12
    s0, la, lb = lo + i_s, lo + ia, lo + ib
    m0, ka, kb = (int(wt[s0]) + 3) % A, (int(wt[la]) + 9) % A, (int(wt[lb]) + 11) % A
    x0 = capped_start(wt, [s0], [m0])
    y = wt.copy(); y[la] = ka
    h, J = m["h"], m["J"].copy()
    g = _grad(J, h, lo, y)                                                  # before the couplings
    zt = depth + MREF_CAP
    c2 = -2.0 * zt - (g[la, ka] - g[la, int(wt[la])])
    c3 = (g[s0, int(wt[s0])] - g[s0, m0]) - 2.0 * (zt - gap)
    assert c2 > 0 and c3 > 0
    _couple(J, ia, ka, i_s, int(wt[s0]), c2)
    _couple(J, ia, ka, i_s, m0, c2 + c3)
    _couple(J, ia, ka, ib, kb, -200.0)
    gy = _grad(J, h, lo, y)
    z = [(gy[la, int(wt[la])] - gy[la, ka]) * np.float32(0.5), (gy[s0, int(wt[s0])] - gy[s0, m0]) * np.float32(0.5)]
    m.update(J=J, x0=x0, spread=spread_of(_grad(J, h, lo, x0), m["lo"], m["hi"]), spread_y=spread_of(gy, 0, L - 1),
             depth=float(max(z) - min(spread_of(gy, 0, L - 1) / 2.0, MREF_CAP)), revert_gap=float(z[0] - z[1]),
             path=(la * A + ka, s0 * A + int(wt[s0])))
    return m


def reverts_only_library(m):
    """The library that leaves open only the two mutated residues of a capped_model, each with its wild-type letter alone: from the
    start state (outside the library) the two reverts are the only admissible moves, with no mutation cap."""
    words = np.zeros(m["L"], np.uint32)
    for p in m["cap_sites"]:
        words[p] = 1 << int(m["wt"][p])
    return words


def oracle_energy(m):
    return _energy(m["J"], m["h"], m["i0"], m["wt"])


# ------------------------------------------------------------------------------------------------ the cells
def _cell(name, model, mode="default", **kw):
    c = dict(name=name, model=model, mode=mode, rng_mode=1, lib=None, betas=None, nmut=0, seed=7000 + len(CELLS), expect="runs",
             policies=(False, True), notrace=False, group="sweep", T=T)
    c.update(kw)
    CELLS.append(c)
    return c


CELLS = []
for _kind, _D in [("within", "tiny"), ("within", 60), ("across", 60), ("within", 127), ("across", 127), ("within", 129), ("across", 129),
                  ("within", 200), ("across", 200), ("within", 290)]:
    _cell(f"sweep:L24:{_kind}:{_D}", ("spread", 24, _D, _kind), notrace=(_kind, _D) == ("across", 200))
for _L in (104, 237):
    for _D in (129, 200):
        _cell(f"sweep:L{_L}:across:{_D}", ("spread", _L, _D, "across"), notrace=_D == 200)
for _D in (129, 200):
    _cell(f"modes:default_lib:{_D}", ("spread", 24, _D, "across"), lib="window", group="modes")
    _cell(f"modes:rev:{_D}", ("spread", 24, _D, "across"), mode="rev", group="modes")
    _cell(f"modes:rev_lib:{_D}", ("spread", 24, _D, "across"), mode="rev", lib="window", group="modes")
    _cell(f"modes:ladder_hot:{_D}", ("spread", 24, _D, "across"), mode="temp", betas=LADDER_HOT, group="modes")
    _cell(f"modes:ladder_control:{_D}", ("spread", 24, _D, "across"), mode="temp", betas=LADDER_CONTROL, group="modes")
# a ladder steep enough for the reference's beta to matter on the overflow side: beta = 3 at spread 96 puts a logit at 144, 80 above
# the reference min(3 x 48, 64) = 64 -- and 96 above a reference formed without beta (48)
_cell("modes:ladder_steep:within:96", ("spread", 24, 96, "within"), mode="temp", betas=(3.0, 1.0), group="modes")
_cell("replay:within:200", ("spread", 24, 200, "within"), rng_mode=0, group="replay")
# proposal range 4 .. 13 inside the Potts window 4 .. 19, the spread planted at residue 16: the forward rows mask it, the reverse
# rows (every residue, no masks) carry a logit of 120 that only the all-residue reference (64, against 20 over the range) keeps finite
_cell("outside:within:240", ("outside", 24, 240), group="outside")
for _d in (-40, -80, -86, -95, -110):
    _cell(f"capped:default:{_d}", ("capped", _d, 1.0), nmut=2, group="capped")
    _cell(f"capped:lib:{_d}", ("capped", _d, 1.0), lib="reverts", group="capped")
# a capped start under a ladder: beta = 1/4 scales the revert logits AND the reference; a reference without beta lies 29 deeper
_cell("capped:ladder:-75", ("capped", -75, 0.25, 400.0), mode="temp", betas=(0.25, 0.125), nmut=2, group="capped")
# capped REVERSE rows of reversible mode (DESIGN.md 4.2b's limit) and a default-mode reverse row past the overflow edge: the large
# spread is in g_y only (planted couplings). The overflow cell runs ONE iteration: an accepted chain's next forward row overflows too
for _d in (-80, -95, -110):
    _cell(f"revcap:{_d}", ("revcap", _d), mode="rev", nmut=2, group="revcap")
_cell("overflow:gy_only:330", ("gy_overflow",), expect="flag", group="overflow", T=1)
# (both policies: the first forward path of either is k_propose's, so this flags in iteration 0 under both; the fused launch's own
#  forward guard -- the same propose_body_dev -- is what flags capped:default:-86 under reuse, whose first abnormal row comes later)
_cell("overflow:within:320", ("spread", 24, 320, "within"), expect="flag", group="overflow")

# Philox keys searched on the CPU (the first of seed, seed + 100, ...) so that no decision of the REFERENCE comes within five times
# the near-tie thresholds: tests/test_chain_range_cpu.py asserts the thresholds themselves for every cell. The price: this matrix never
# puts the device AT a near-tie; how a parted chain is vetted there is exercised by tests/test_modes_gpu.py and the fuzz runs
SEEDS = {"sweep:L24:within:tiny": 7300, "sweep:L24:across:60": 7102, "sweep:L24:across:127": 7104, "sweep:L104:across:200": 7111,
         "modes:rev:200": 7120, "modes:ladder_hot:200": 7322, "modes:ladder_control:200": 7123}
for _c in CELLS:
    _c["seed"] = SEEDS.get(_c["name"], _c["seed"])
CELL = {c["name"]: c for c in CELLS}
# the cells that meet a forward row without (enough) mass somewhere along their path: derived by expected(), asserted equal to it by
# tests/test_chain_range_cpu.py; listed so that the GPU module can name its cases without running the classification at import
FLAGGED = ("capped:default:-86", "capped:default:-95", "capped:lib:-95", "capped:default:-110", "capped:lib:-110", "revcap:-95", "revcap:-110",
           "overflow:gy_only:330", "overflow:within:320")
_MODELS = {}


def cell_model(c):
    key = c["model"]
    if key not in _MODELS:
        if key[0] == "spread":
            _MODELS[key] = spread_model(key[1], SIZES[key[1]], key[2], key[3])
        elif key[0] == "capped":
            _MODELS[key] = capped_model(key[1], beta=key[2], base=key[3] if len(key) > 3 else 280.0)
        elif key[0] == "gy_overflow":
            _MODELS[key] = gy_overflow_model()
        elif key[0] == "revcap":
            _MODELS[key] = capped_reverse_model(key[1])
        elif key[0] == "outside":
            m = spread_model(key[1], SIZES[key[1]], 40, "across")            # (the window's own spread stays small: 40)
            lo = m["lo"]
            g0 = _grad(m["J"], m["h"], lo, m["wt"])
            l, h = lo + 12, m["h"].copy()
            k = (int(m["wt"][l]) + 7) % A
            h[12, k] += np.float32(key[2] / 2.0 - g0[l, k])
            h[12, int(m["wt"][l])] -= np.float32(key[2] / 2.0 + g0[l, int(m["wt"][l])])
            m.update(h=h, hi=lo + 9, outside=(l, k))
            g = _grad(m["J"], h, lo, m["wt"])
            m["spread"] = spread_of(g, m["lo"], m["hi"])
            m["spread_all"] = spread_of(g, 0, m["L"] - 1)
            _MODELS[key] = m
    return _MODELS[key]


def cell_setup(c):
    """(model dict, library words or None, start states int64 [N, L], nmut) of a cell."""
    m = cell_model(c)
    lib = None
    if c["lib"] == "window":
        lib = dl.fold_range(hl.seeded_library(m["wt"], m["lo"], m["hi"], seed=41), m["lo"], m["hi"])
    elif c["lib"] == "reverts":
        lib = reverts_only_library(m)
    start = m["wt"] if m.get("x0") is None else m["x0"]
    return m, lib, np.tile(np.asarray(start).astype(np.int64), (N, 1)), c["nmut"]


def cell_noise(c, m):
    """The device RNG's draws of the cell restated on the CPU (orc.device_noise), or torch's for the replay control."""
    if c["rng_mode"] == 0:
        gen = torch.Generator().manual_seed(c["seed"])
        return [orc.draw_noise_torch(N, m["L"] * A, PAS, generator=gen) for _ in range(c["T"])]
    return [orc.device_noise(c["seed"], 0, N, t, PAS, m["L"]) for t in range(c["T"])]


def reference_run(c, energy, noise, keep_probs=True, emulate=False):
    """The fp32 reference of the cell's mode on `energy` and explicit noise (traced). emulate: called inside emulated(c), which applies
    the library itself (helpers_library.masked_oracle would put its own rows in front of the emulation's)."""
    m, lib, x0, nmut = cell_setup(c)
    fn = lambda t: noise[t]
    if c["mode"] == "default":
        if lib is None or emulate:
            return orc.run(energy, x0, m["wt"], fn, len(noise), m["lo"], m["hi"], PAS, nmut, False, trace=True, keep_probs=keep_probs)
        return hl.masked_run(lib, energy, x0, m["wt"], fn, len(noise), m["lo"], m["hi"], PAS, nmut, False, trace=True, keep_probs=keep_probs)
    if c["mode"] == "rev":
        return hr.reversible_run(energy, x0, m["wt"], fn, len(noise), m["lo"], m["hi"], PAS, nmut, trace=True, keep_probs=keep_probs, allowed=lib)
    return ht.tempered_run(energy, x0, m["wt"], fn, len(noise), m["lo"], m["hi"], PAS, nmut, c["betas"], 1, seed=c["seed"], allowed=lib,
                           trace=True, keep_probs=keep_probs)


def as_trace(ref, noise):
    """What score() reads of a run, from a reference run: dict(flat [T, mu, n], U [T, n], accepted [T, n], rung_history or None)."""
    mu = 2 * PAS - 1
    n = ref["accepted"].shape[1]
    flat = np.zeros((len(noise), mu, n), np.int64)
    for t, out in enumerate(ref["traces"]):
        f = out["flat"].numpy()
        flat[t, :f.shape[0]] = f
    return dict(flat=flat, U=np.stack([nz[0].numpy() for nz in noise]), accepted=ref["accepted"].numpy().astype(bool),
                rung_history=ref.get("rung_history"))


# ------------------------------------------------------------------------------------------------ scoring a recorded path
class CastEnergy:
    """An energy adaptor's outputs in another dtype (.double() for the fp64 score): the oracle's functions follow the dtype."""

    def __init__(self, energy, dtype):
        self.energy_fn, self.dtype = energy, dtype

    def energy(self, idx):
        e, f = self.energy_fn.energy(idx)
        return e.to(self.dtype), f.to(self.dtype)

    def energy_grad(self, idx):
        e, f, g = self.energy_fn.energy_grad(idx)
        return e.to(self.dtype), f.to(self.dtype), g.to(self.dtype)


@contextlib.contextmanager
def recorded_draws():
    """Inside the block orc.race_sample returns the recorded draw it is handed in place of the race variates."""
    orig = orc.race_sample
    orc.race_sample = lambda p_hat, q: q.long()
    try:
        yield
    finally:
        orc.race_sample = orig


def score(c, energy, trace, dtype=torch.float64, start=None, emulate=False):
    """The accept log-ratio of every iteration of a recorded run of cell `c` -- trace = dict(flat, U, accepted[, rung_history]) as
    Chains.trace() returns them (+ Chains.tempering_history()) -- along that run's OWN path: the draws are the recorded ones, the
    accept bits are imposed (u = 0 / inf), the rows, log-probabilities and the ratio come from the reference's iteration function of
    the cell's mode on `energy`'s outputs cast to `dtype`. Returns dict(log_acc [T, n] fp64, de [T, n] = (beta) (e_y - e_x),
    mismatch = the iterations x chains whose imposed accept the mode's rule refuses). emulate: the rows are formed by
    fixed_reference_fp32 (the emulated() context) instead."""
    m, lib, x0, nmut = cell_setup(c)
    wt = torch.as_tensor(m["wt"].astype(np.int64))
    thr = np.iinfo(np.int32).max if nmut == 0 else nmut
    cur = torch.as_tensor(x0 if start is None else start).long()
    en = CastEnergy(energy, dtype)
    la, de, bad = [], [], []
    full = dl.full_library(m["L"]) if lib is None else lib
    if emulate:
        rows = emulated(c)
    else:
        rows = hl.masked_oracle(lib) if (c["mode"] == "default" and lib is not None) else contextlib.nullcontext()
    with recorded_draws(), rows:
        for t in range(trace["U"].shape[0]):
            U = torch.as_tensor(trace["U"][t]).long()
            q = torch.as_tensor(np.maximum(trace["flat"][t][:int(U.max())], 0))          # (inactive sub-steps hold -1: never applied)
            acc = torch.as_tensor(trace["accepted"][t].astype(bool))
            u = torch.where(acc, torch.zeros(()), torch.full((), math.inf)).to(torch.float32)
            if c["mode"] == "default":
                out = orc.pas_iteration(en, cur, cur, wt, U, q, u, m["lo"], m["hi"], thr)
            else:
                beta = np.asarray(c["betas"], np.float32)[trace["rung_history"][t]] if c["mode"] == "temp" else 1.0
                e_it = ht.ScaledEnergy(en, beta)                             # (beta = 1 keeps every bit)
                out = hr.reversible_iteration(e_it, cur, cur, wt, U, q, u, m["lo"], m["hi"], thr, full)
            bad.append((out["accepted"] != acc).numpy())
            la.append(out["log_acc"].double().numpy())
            de.append((out["e_y"] - out["e_x"]).double().numpy())
            cur = torch.where(acc.reshape(-1, 1), out["proposal"], cur)
            if c["mode"] == "default":
                cur[(cur != wt.reshape(1, -1)).sum(-1) >= thr] = wt
    return dict(log_acc=np.stack(la), de=np.stack(de), mismatch=np.stack(bad))


def score64(c, energy, trace, start=None):
    return score(c, energy, trace, torch.float64, start)


def log_acc_error(a, b):
    """|a - b| where both are finite, 0 where both are the same infinity, inf otherwise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both = np.isfinite(a) & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        return np.where(both, np.abs(a - b), np.where(a == b, 0.0, np.inf))


def outer_bound(la64, de64):
    """2e-4 + 2^-23 (|e_y - e_x| + |log_acc|): the project's log_acc tolerance and the two fp32 roundings of fl(fl(beta (e_y - e_x)) + ratio)."""
    with np.errstate(invalid="ignore"):
        return 2e-4 + 2.0 ** -23 * (np.abs(de64) + np.where(np.isfinite(la64), np.abs(la64), 0.0))


def inner_bound(yardsticks, U):
    """DESIGN.md 5's rule: 4 x the larger yardstick of the cell + one fp32 ulp of 16 = -log 2^-23 (the largest term) per sub-step."""
    return 4.0 * max(yardsticks) + 16.0 * 2.0 ** -23 * np.asarray(U, np.float64)


# ------------------------------------------------------------------------------------------------ the device's row arithmetic in fp32
def _tree(v):
    """wave_sum / row8_sum (common.h): a balanced binary tree over a power-of-two number of lanes in lane order."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _sum_wave0(e):
    """propose_body_dev's total_mass / S3 of wave 0: e fp32 [n, L, 20] -> (residue masses [n, L], total [n]). Per residue the fixed tree
    ((e0..3 + e4..7) + (e8..11 + e12..15)) + e16..19 then (x + y) + (z + w); lane l % 64 adds its residues in order; wave tree."""
    t = ((e[..., 0:4] + e[..., 4:8]) + (e[..., 8:12] + e[..., 12:16])) + e[..., 16:20]
    mass = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    n, L = mass.shape
    lanes = np.zeros((n, 64), np.float32)
    for r in range((L + 63) // 64):
        part = mass[:, 64 * r:64 * (r + 1)]
        lanes[:, :part.shape[1]] += part
    return mass, _tree(lanes)


def _sum_block(e):
    """reverse_rows_dev's row sums over the workgroup: e fp32 [n, N]; thread t adds the entries of its groups t + 512 r in order, then
    the wave tree, then the tree over the 8 waves."""
    n, N = e.shape
    n4 = N // 4
    th = np.zeros((n, 512), np.float32)
    for r in range((n4 + 511) // 512):
        g = e[:, 2048 * r:2048 * (r + 1)].reshape(n, -1, 4)
        s = th[:, :g.shape[1]]
        for i in range(4):
            s = s + g[:, :, i]
        th[:, :g.shape[1]] = s
    return _tree(_tree(th.reshape(n, 8, 64)))


def classify(S1):
    """The class of a normaliser: normal, denormal (0 < S1 < 2^-126), recip_inf (1 / S1 overflows), zero, inf (or NaN)."""
    S1 = np.asarray(S1, np.float32)
    with np.errstate(divide="ignore", over="ignore"):
        rinf = np.isinf(np.float32(1.0) / S1)
    out = np.full(S1.shape, "normal", dtype=object)
    out[(S1 > 0) & (S1 < np.float32(2.0 ** -126))] = "denormal"
    out[(S1 > 0) & rinf] = "recip_inf"
    out[S1 == 0] = "zero"
    out[~(S1 < np.inf) | (S1 < 0)] = "inf"
    return out


def _clamp(p):
    """v_med3_f32(p, 2^-23, 1 - 2^-23) and clampp(): a NaN gives the minimum of the other two."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p), EPS, np.minimum(np.maximum(p, EPS), ONE_M)).astype(np.float32)


def fixed_reference_fp32(z_row, mref, masks=None, lib=None, layout="wave0", guard="window", S1_carried=None):
    """One row of the device-RNG kernels in numpy float32, for n chains at once. z_row fp32 [n, L * 20] logits, masks bool [n, L * 20]
    (True = masked by the range or the cap: e = 0; a -inf logit counts as masked), mref fp32 [n], lib bool [L * 20] or [n, L * 20]
    (True = allowed) or None. e = exp(z - mref); S1 = the fixed tree of the layout ("wave0": total_mass of propose_body_dev, "block":
    the workgroup sum of reverse_rows_dev); c = 1 / S1; p = med3(e c, 2^-23, 1 - 2^-23) (a NaN gives the minimum of the other two);
    forbidden entries 0; residue masses and S3 by the same trees. guard, what happens to an S1 that is not in [2^-125, inf):
      "window"  flagged, S1 := 1 (forward rows: PPDE_ERR_NUMERIC; reversible reverse rows: the path is rejected, and `window` marks
                the rows the device also reports as PPDE_ERR_NUMERIC: the ones that hold an admissible entry at all);
      "inf"     (default-mode reverse rows) only a non-finite S1 is reported (`window`); S1 is used as it is;
      "zero"    only S1 = 0 or non-finite is flagged, S1 := 1 (the kernels before the window was closed);
      None      nothing (default-mode reverse rows: S1 as it is).
    S1_carried: a normaliser to use in place of the re-summed one (planted fault).
    Returns dict(p [n, L * 20] clamped and zeroed, e, S1, S3, cls (of S1), flagged, window)."""
    z = np.asarray(z_row, np.float32)
    n, Nn = z.shape
    mref = np.broadcast_to(np.asarray(mref, np.float32), (n,)).copy()
    dead = np.isneginf(z) if masks is None else (np.asarray(masks, bool) | np.isneginf(z))
    allowed = np.ones((n, Nn), bool) if lib is None else np.broadcast_to(np.asarray(lib, bool), (n, Nn))
    dead = dead | ~allowed

    def exps(ref):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return np.where(dead, np.float32(0), np.exp((np.where(dead, np.float32(0), z) - ref[:, None]).astype(np.float32))).astype(np.float32)

    def summed(e):
        with np.errstate(over="ignore", invalid="ignore"):
            return (_sum_wave0(e.reshape(n, -1, A))[1] if layout == "wave0" else _sum_block(e)).astype(np.float32)

    e = exps(mref)
    S1 = summed(e) if S1_carried is None else np.asarray(S1_carried, np.float32).copy()
    first = S1.copy()
    window = np.zeros(n, bool)
    if guard == "window":
        bad = ~((S1 >= S1_MIN) & (S1 < np.inf))
        window = bad & ((~dead).any(-1) | (S1 != 0))
    elif guard == "zero":
        bad = ~((S1 > 0) & (S1 < np.inf))
    elif guard == "inf":
        bad = np.zeros(n, bool)
        window = ~(S1 < np.inf)
    else:
        bad = np.zeros(n, bool)
    S1c = np.where(bad, np.float32(1), S1).astype(np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        c = (np.float32(1.0) / S1c).astype(np.float32)
        p = _clamp((e * c[:, None]).astype(np.float32))
    p = np.where(allowed, p, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        S3 = _sum_wave0(p.reshape(n, -1, A))[1] if layout == "wave0" else _sum_block(p)
    return dict(p=p, e=e, S1=first, S3=S3.astype(np.float32), cls=classify(first), flagged=bad, window=window)


FAULTS = ("mref_uncapped", "mref_without_beta", "S1_carried", "reverse_mref_over_range", "unguarded_window")


@contextlib.contextmanager
def emulated(c, fault=None, log=None):
    """Inside the block the reference's iteration functions of cell `c`'s mode form every proposal row with fixed_reference_fp32: the
    forward rows against mref = min(beta spread(g_x over the range) / 2, 64) in wave 0's trees, the reverse rows against mref over every
    residue of g_y in the workgroup's trees (default mode: no masks; reversible: the forward row function, a row without mass rejects
    the path). A forward row without mass raises NumericFlag, as the device flags PPDE_ERR_NUMERIC. `log` (a list) receives
    (phase, cls [n], S1 [n], z_max - mref [n]) of every row. `fault` plants one of FAULTS:
      mref_uncapped            no cap at 64;
      mref_without_beta        spread / 2 under a ladder, where beta spread / 2 is meant;
      S1_carried               forward rows: S1 += sum(e_new - e_old) over the entries the last move changed, instead of the fresh sum;
      reverse_mref_over_range  the reverse rows' reference taken over the proposal range;
      unguarded_window         c = 1 / S1 down to S1 = 0: where 1 / S1 overflows every admissible entry becomes 1 - 2^-23 and
                               nothing is flagged (the kernels before the window was closed)."""
    m, lib, _, _ = cell_setup(c)
    lo, hi, L = m["lo"], m["hi"], m["L"]
    cap = np.inf if fault == "mref_uncapped" else MREF_CAP
    st = dict(beta=None, phase="fwd", prev=None)
    guard = "zero" if fault == "unguarded_window" else "window"

    def mref_of(grad, fwd):
        g = grad.detach().numpy().astype(np.float32)
        if fwd or fault == "reverse_mref_over_range":
            g = g[:, lo:hi + 1]
        g = g.reshape(g.shape[0], -1)
        half = (g.max(-1) - g.min(-1)) * np.float32(0.5)
        if fault == "mref_without_beta" and st["beta"] is not None:
            half = half / st["beta"]
        return np.minimum(np.maximum(half, np.float32(0)), np.float32(cap)).astype(np.float32)

    def note(phase, r, z, mref):
        if log is not None:
            with np.errstate(invalid="ignore"):
                log.append((phase, r["cls"], r["S1"], np.where(np.isneginf(z), -np.inf, z).max(-1) - mref))

    def forward_row(z, grad, forbid):
        z = z.numpy().astype(np.float32)
        mref = mref_of(grad, True)
        allowed = None if forbid is None else ~forbid.numpy().reshape(-1)
        carried = None
        if fault == "S1_carried" and st["prev"] is not None:
            e_old, S_old = st["prev"]
            e_new = fixed_reference_fp32(z, mref, lib=allowed, guard=None)["e"]
            d = (e_new.reshape(len(z), L, A) - e_old.reshape(len(z), L, A)).astype(np.float32)
            carried = (S_old + _sum_wave0(d)[1]).astype(np.float32)
        r = fixed_reference_fp32(z, mref, lib=allowed, guard=guard, S1_carried=carried)
        if fault == "S1_carried":
            st["prev"] = (r["e"], r["S1"])
        note("fwd", r, z, mref)
        if r["flagged"].any():
            raise NumericFlag(f"forward row without mass: chains {np.flatnonzero(r['flagged']).tolist()}")
        return torch.as_tensor(r["p"] / r["S3"][:, None])

    def reverse_row(z, grad, forbid, rev):
        z = z.numpy().astype(np.float32)
        mref = mref_of(grad, False)
        allowed = None if forbid is None else ~forbid.numpy().reshape(-1)
        r = fixed_reference_fp32(z, mref, lib=allowed, layout="block", guard=("zero" if rev else None) if fault == "unguarded_window" else ("window" if rev else "inf"))
        note("rev", r, z, mref)
        if r["window"].any():
            raise NumericFlag(f"reverse row without usable mass: chains {np.flatnonzero(r['window']).tolist()}")
        return torch.as_tensor(r["p"] / r["S3"][:, None]), torch.as_tensor(r["flagged"])

    orig_fl, orig_pl, orig_cp, orig_row, orig_scaled = orc.forward_logits, orc.path_logits, orc.categorical_probs, hr.proposal_row, ht.ScaledEnergy
    pend = dict(grad=None, fwd=False)
    forbid_default = None if lib is None else torch.as_tensor(~dl.as_bool(lib)).reshape(1, -1)

    def path_logits(grad, idx):
        if pend.get("nested"):
            return orig_pl(grad, idx)
        pend.update(grad=grad, fwd=False)
        if st["phase"] == "fwd":                                             # the first reverse row of an iteration: a new forward path follows
            st["phase"] = "rev"
        return orig_pl(grad, idx)

    def forward_logits(grad, idx, *a, **k):
        pend["nested"] = True
        z = orig_fl(grad, idx, *a, **k)
        pend["nested"] = False
        if st["phase"] == "rev":
            st.update(phase="fwd", prev=None)
        pend.update(grad=grad, fwd=True)
        return z if forbid_default is None else torch.where(forbid_default, torch.tensor(-math.inf), z)

    def categorical_probs(z):                                                # default mode (orc.pas_iteration)
        if pend["fwd"]:
            return forward_row(z, pend["grad"], forbid_default)
        return reverse_row(z, pend["grad"], None, False)[0]

    calls = dict(n=0, fwd=True)

    def proposal_row(grad, state, wt_idx, min_pos, max_pos, thr, forbid):      # reversible mode (hr.reversible_iteration)
        pend["nested"] = True
        z = orig_fl(grad, state, wt_idx, min_pos, max_pos, thr)
        pend["nested"] = False
        z = torch.where(forbid, torch.tensor(-math.inf), z)
        if calls["fwd"]:
            return forward_row(z, grad, forbid), torch.zeros(z.shape[0], dtype=torch.bool)
        return reverse_row(z, grad, forbid, True)

    class PhaseEnergy(orig_scaled):
        """ScaledEnergy that tells the emulation its beta and which phase of the iteration the rows belong to (the x call opens the
        forward path, the y call the reverse one)."""

        def energy_grad(self, idx):
            calls["n"] += 1
            calls["fwd"] = calls["n"] % 2 == 1
            if calls["fwd"]:
                st["prev"] = None
            st["beta"] = self.beta.numpy().astype(np.float32) if self.beta.ndim else None
            return super().energy_grad(idx)

    orc.forward_logits, orc.path_logits, orc.categorical_probs = forward_logits, path_logits, categorical_probs
    hr.proposal_row, ht.ScaledEnergy = proposal_row, PhaseEnergy
    try:
        yield PhaseEnergy
    finally:
        orc.forward_logits, orc.path_logits, orc.categorical_probs = orig_fl, orig_pl, orig_cp
        hr.proposal_row, ht.ScaledEnergy = orig_row, orig_scaled


def emulated_energy(c, energy, wrap):
    """The energy to hand an emulated run: reversible cells need the phase-telling wrapper (beta 1 keeps every bit)."""
    return wrap(energy, 1.0) if c["mode"] == "rev" else energy


_EXPECTED = {}


def expected(c):
    """What the device must do in a cell, derived on the CPU: "flag" (PPDE_ERR_NUMERIC at sync) when the emulated run on the CPU oracle
    meets a forward row whose normaliser is below 2^-125 or non-finite, "runs" (and agrees with the reference) otherwise."""
    if c["name"] not in _EXPECTED:
        m = cell_model(c)
        try:
            with emulated(c) as wrap:
                reference_run(c, emulated_energy(c, oracle_energy(m), wrap), cell_noise(c, m), keep_probs=False, emulate=True)
            _EXPECTED[c["name"]] = "runs"
        except NumericFlag:
            _EXPECTED[c["name"]] = "flag"
    return _EXPECTED[c["name"]]

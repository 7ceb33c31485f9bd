"""Helpers of the expert-set x mode matrix (tests/test_modes_cpu.py, tests/test_modes_gpu.py): library, reversible and tempering
runs on the supervised expert alone (which = 2), on the transformer expert (which = 5, 6, 7) and with the full gradient (| 8).

`DeviceEnergy(model, which)` gives the CPU references (orc.run, helpers_library.masked_run, helpers_reversible.reversible_run,
helpers_tempering.tempered_run and the enumerated kernels) the numbers the chain kernels read: it has the oracle's interface and
serves `model.energy_grad(x, which)`. A chain's energy, fitness and gradient do not depend on the batch it is evaluated in
(tests/test_transformer_gpu.py, tests/test_hip_shapes.py hold that bit for bit), so what is left to differ between such a
reference and a device run is the chain kernels' own fp32 arithmetic; the experts' arithmetic stays pinned where it is.

`OracleModel` is the stand-in the CPU tests put under the adaptor: the same `energy_grad(idx, which, want_grad)` served by the CPU
oracle (Potts, CNN ensemble, esm_oracle.TransformerDelta), with the device's meaning of `which`.

`compare_replay` is the ONE comparison both modules use: the GPU module hands it a device run, the CPU module a reference run in
the device's layout against a reference with a planted fault."""
import contextlib

import numpy as np
import torch

import helpers_library as hl
import helpers_reversible as hr
import helpers_tempering as ht
import ppde_oracle as orc
from helpers import compare_runs_up_to_near_ties
from ppde_amd import library as dl
from ppde_amd import synthetic

A = 20
GAP_TOL, ACC_TOL = 1e-5, 2e-4                  # the project's fp32 near-tie thresholds: race gap, |log_acc - log u|
LOG_ACC_TOL, E_TOL, F_TOL = 2e-4, 2e-5, 5e-6   # log_acc absolute; histories relative to max(1, |value|)
N, T, PAS, NMUT, LAMDA = 16, 20, 2, 3, 2.0
WHICH = (2, 5, 6, 7, 7 | 8)
MODES = ("default_lib", "rev", "rev_lib", "temp_sw1", "temp_sw2", "temp_lib")
BETAS = ht.REPLAY_BETAS
TOY = dict(L=24, win=(4, 16), layers=2, dim=128, heads=4, ffn=256, seed=3)      # tests/test_transformer_gpu.py's _model(...)
LARGE = ((104, (23, 76)), (237, (0, 237)))     # two and three groups per thread
N_LARGE, T_LARGE = 8, 6


class DeviceEnergy:
    """The oracle's interface over `model.energy_grad(idx uint8 [n, L], which, want_grad)`: energy(idx) -> (e, fit),
    energy_grad(idx) -> (e, fit, g); int64 CPU tensors in, fp32 CPU tensors out, in the oracle's shapes."""

    def __init__(self, model, which):
        self.model, self.which = model, int(which)

    def _eval(self, idx, want_grad):
        x = torch.as_tensor(np.asarray(idx)).to(torch.uint8).contiguous()
        e, fit, g = self.model.energy_grad(x, self.which, want_grad)
        return e.cpu(), fit.cpu(), (g.cpu() if g is not None else None)

    def energy(self, idx):
        e, fit, _ = self._eval(idx, False)
        return e, fit

    def energy_grad(self, idx):
        return self._eval(idx, True)


class OracleModel:
    """`energy_grad(idx, which, want_grad)` of the HIP model, served by the CPU oracle: bit 0 Potts, bit 1 the supervised
    ensemble, bit 2 the transformer, bit 3 the full gradient; which = 2 is ProteinSupervised, e = fit and g = d fit / dx."""

    def __init__(self, potts, cnn, tf, lamda):
        self.potts, self.cnn, self.tf, self.lamda = potts, cnn, tf, float(lamda)

    def energy_grad(self, idx, which, want_grad=True):
        idx = torch.as_tensor(np.asarray(idx)).long()
        if which & 7 == 2:
            fit, g = self.cnn.fit_grad(idx, want_grad=want_grad)
            return fit, fit, g
        en = orc.EnergyOracle(self.potts if which & 1 else None, self.cnn if which & 2 else None, self.lamda,
                              tf=self.tf if which & 4 else None, full_grad=bool(which & 8))
        if want_grad:
            return en.energy_grad(idx)
        return en.energy(idx) + (None,)


def toy_parts(L=TOY["L"], win=TOY["win"], seed=TOY["seed"]):
    """(wt, J, h, cnn states, ESM-2 state) of tests/test_transformer_gpu.py's _model(L, 2, 128, 4, 256, with_cnn=True, potts=win)."""
    wt = np.random.default_rng(seed).integers(0, 20, L).astype(np.uint8)
    J, h = synthetic.make_potts(win[1], seed=seed)
    cnn = [synthetic.make_cnn_state(L, s) for s in range(3)]
    st = synthetic.make_esm2_state(TOY["layers"], TOY["dim"], TOY["heads"], TOY["ffn"], seed=seed)
    return wt, J, h, cnn, st


CPU_TF = dict(layers=1, dim=64, heads=4, ffn=128)       # the CPU stand-in's transformer: toy sizes, the suite runs it ~2000 times


def oracle_model(L=TOY["L"], win=TOY["win"], cnn_gain=1.0):
    """The CPU stand-in of the GPU module's model and its wild type: the same wild type, Potts couplings and CNNs, a smaller
    seeded transformer (fp16 rounding points as on the device)."""
    import esm_oracle as eo
    wt, J, h, cnn, _ = toy_parts(L, win)
    cnn = scaled_cnn(cnn, cnn_gain)
    st = synthetic.make_esm2_state(CPU_TF["layers"], CPU_TF["dim"], CPU_TF["heads"], CPU_TF["ffn"], seed=TOY["seed"])
    esm = eo.EsmOracle(st, CPU_TF["layers"], CPU_TF["dim"], CPU_TF["heads"], half_points=True)
    P = orc.PottsOracle(J, h, win[0], torch.as_tensor(wt.astype(np.int64)))
    return OracleModel(P, orc.CnnOracle(cnn), eo.TransformerDelta(esm, wt), LAMDA), wt


def scaled_cnn(cnn, gain):
    """The networks with their output layer scaled: fit -> gain * fit (a power of two keeps every rounding in place)."""
    return [dict(sd, **{"decoder.weight": sd["decoder.weight"] * np.float32(gain), "decoder.bias": sd["decoder.bias"] * np.float32(gain)})
            for sd in cnn]


def window_library(wt, win, seed=41):
    lo, hi = win[0], win[0] + win[1] - 1
    return dl.fold_range(hl.seeded_library(wt, lo, hi, seed=seed), lo, hi)


def one_site_library(wt, site, letters=A, seed=31):
    """One open residue with `letters` letters, the wild type's among them (helpers_tempering.one_site_case's library)."""
    rng = np.random.default_rng(seed)
    allowed = np.zeros(len(wt), np.uint32)
    others = [k for k in rng.permutation(A).tolist() if k != int(wt[site])][:letters - 1]
    allowed[site] = sum(1 << k for k in others) | (1 << int(wt[site]))
    return allowed


# Philox keys of the which = 2 ladder cells (see tests/test_modes_gpu.py's header): searched on the CPU stand-in for a run that
# refuses a swap, shows a swap decided on fit * lamda in its rung history and keeps tests/test_tempering_cpu.py's margins
PHILOX_SEEDS = {(2, "temp_sw1"): 3103}


def philox_seed(which, mode):
    return PHILOX_SEEDS.get((int(which), mode), 1000 + 37 * int(which) + MODES.index(mode))


def torch_noise(which, mode, n, L, T_=T, pas=PAS):
    gen = torch.Generator().manual_seed(5000 + philox_seed(which, mode))
    return [orc.draw_noise_torch(n, L * A, pas, generator=gen) for _ in range(T_)]


def mode_settings(mode, lib):
    """(library or None, reversible, betas or None, swap_every) of a mode."""
    return (lib if mode.endswith("lib") else None, mode != "default_lib", BETAS if mode.startswith("temp") else None,
            2 if mode == "temp_sw2" else 1)


def reference_run(mode, energy, wt, lib, noise, win, seed, n=N, nmut=NMUT, pas=PAS):
    """The CPU iteration of `mode` on `energy` and explicit noise, from the wild type, traced with its proposal rows."""
    lo, hi = win[0], win[0] + win[1] - 1
    x0 = np.tile(np.asarray(wt).astype(np.int64), (n, 1))
    use_lib, _, betas, swap_every = mode_settings(mode, lib)
    fn = lambda t: noise[t]
    if mode == "default_lib":
        return hl.masked_run(lib, energy, x0, wt, fn, len(noise), lo, hi, pas, nmut, False, trace=True, keep_probs=True)
    if betas is None:
        return hr.reversible_run(energy, x0, wt, fn, len(noise), lo, hi, pas, nmut, trace=True, keep_probs=True, allowed=use_lib)
    return ht.tempered_run(energy, x0, wt, fn, len(noise), lo, hi, pas, nmut, betas, swap_every, seed=seed, allowed=use_lib,
                           trace=True, keep_probs=True)


def as_device_run(ref, noise, mu_max):
    """A reference run in the layout a device run is read in: dict(tr, res, temp)."""
    T_, n = len(noise), ref["energy_history"].shape[1]
    flat = np.zeros((T_, mu_max, n), np.int32)
    for t, out in enumerate(ref["traces"]):
        f = out["flat"].numpy()
        flat[t, :f.shape[0]] = f
    tr = dict(flat=flat, accepted=ref["accepted"].numpy().astype(np.uint8),
              log_acc=np.stack([o["log_acc"].numpy() for o in ref["traces"]]), U=np.stack([nz[0].numpy() for nz in noise]).astype(np.int32))
    res = dict(energy_history=ref["energy_history"].numpy(), fitness_history=ref["fitness_history"].numpy(),
               best_idx=ref["best_idx"].numpy().astype(np.uint8), random_traj=ref["states"][:, 0].numpy().astype(np.uint8))
    temp = None
    if "rung_history" in ref:
        temp = dict(hist=ref["rung_history"], rung=ref["rung"], beta=ref["beta"], swap_attempts=ref["swap_attempts"],
                    swap_accepts=ref["swap_accepts"])
    return dict(tr=tr, res=res, temp=temp)


def margins(noise, ref):
    """(smallest |log_acc - log u| over the decisions u takes, smallest race gap) of a reference run of any mode."""
    for out in ref["traces"]:
        out.setdefault("refused", torch.zeros_like(out["accepted"]))
    return hr.replay_margins(noise, ref)


def _first_difference(tr, ref, noise, cols):
    for t in range(tr["accepted"].shape[0]):
        U = noise[t][0].numpy()[cols]
        out = ref["traces"][t]
        for s in range(int(noise[t][0].max())):
            act = s < U
            if (tr["flat"][t, s][cols][act] != out["flat"][s].numpy()[cols][act]).any():
                return t
        if (tr["accepted"][t][cols].astype(bool) != out["accepted"].numpy()[cols]).any():
            return t
    return None


def near_ties(tr, ref, noise, R=1):
    """helpers.compare_runs_up_to_near_ties for chains that are coupled in ensembles of R consecutive chains (tempering: a swap
    carries one chain's parting to its neighbours): an ensemble is compared up to and including the iteration of its first
    difference, which must be a near-tie of the reference's own decision, and not after it. R = 1: the helper itself.
    Returns (mask of the chains equal to the end, notes)."""
    n = tr["accepted"].shape[1]
    if R == 1:
        _, notes, same = compare_runs_up_to_near_ties(tr, ref, noise, GAP_TOL, ACC_TOL)
        return same, notes
    same, notes = np.ones(n, bool), []
    for first in range(0, n, R):
        cols = np.arange(first, first + R)
        t_diff = _first_difference(tr, ref, noise, cols)
        if t_diff is None:
            continue
        upto = t_diff + 1
        sub_tr = dict(flat=tr["flat"][:upto][:, :, cols], accepted=tr["accepted"][:upto][:, cols])
        tc = torch.as_tensor(cols)
        sub_ref = dict(traces=[dict(flat=o["flat"][:, tc], p_fwd=o["p_fwd"][:, tc], accepted=o["accepted"][tc],
                                    log_acc=o["log_acc"][tc]) for o in ref["traces"][:upto]])
        sub_noise = [(U[tc], q[:, tc], u[tc]) for U, q, u in noise[:upto]]
        _, sub_notes, _ = compare_runs_up_to_near_ties(sub_tr, sub_ref, sub_noise, GAP_TOL, ACC_TOL)
        assert sub_notes, "a difference the near-tie comparison did not see"
        same[cols] = False                                                   # the whole ensemble leaves the comparison
        notes += [(int(cols[b]), t, what, margin) for b, t, what, margin in sub_notes]
    return same, notes


def _ratio(err, tol):
    return float(np.max(np.asarray(err, np.float64) / np.asarray(tol, np.float64))) if np.size(err) else 0.0


def compare_replay(tag, dev, ref, noise, R=1, record=None, check_U=True, lib=None):
    """A run in the device's layout (dict(tr, res, temp)) against the reference run of the same mode on the same noise.
    Draws and accept bits equal, except that a chain (with tempering: its ensemble) may part at a near-tie of the reference's own
    decision; for the chains that stay: log_acc within 2e-4, energy and fitness histories within 2e-5 max(1, |e|) and
    5e-6 max(1, |f|), best states and the recorded trajectory equal, and with tempering the rung history, final rungs and
    temperatures and both swap counters equal. `record(tag, err, tol)` notes each ratio (tests/test_hip_parity.observed).
    Returns dict(parted, notes, log_acc, energy, fitness, bit_equal)."""
    tr, res = dev["tr"], dev["res"]
    T_, n = tr["accepted"].shape
    if check_U:
        assert np.array_equal(tr["U"], np.stack([nz[0].numpy() for nz in noise])), f"{tag}: path lengths differ"
    same, notes = near_ties(tr, ref, noise, R)
    for note in notes:
        print(f"[modes] {tag}: chain {note[0]} parted at iteration {note[1]} ({note[2]}), margin {note[3]:.3e}")
    if lib is not None:
        ok = dl.as_bool(lib).reshape(-1)
        for t in range(T_):
            U = noise[t][0].numpy()
            for s in range(int(U.max())):
                assert ok[tr["flat"][t, s][s < U]].all(), f"{tag}: a forbidden move was drawn"
    ref_la = np.stack([o["log_acc"].numpy() for o in ref["traces"]])[:, same]
    la = tr["log_acc"][:, same]
    both = np.isfinite(ref_la) & np.isfinite(la)
    with np.errstate(invalid="ignore"):
        err_la = np.where(both, np.abs(la - ref_la), np.where(la == ref_la, 0.0, np.inf))
    eh, fh = ref["energy_history"].numpy()[:, same], ref["fitness_history"].numpy()[:, same]
    de, df = np.abs(res["energy_history"][:, same] - eh), np.abs(res["fitness_history"][:, same] - fh)
    tol_e, tol_f = E_TOL * np.maximum(1.0, np.abs(eh)), F_TOL * np.maximum(1.0, np.abs(fh))
    bit_equal = bool(np.array_equal(res["energy_history"][:, same], eh) and np.array_equal(res["fitness_history"][:, same], fh))
    rec = record if record is not None else (lambda name, err, tol: _ratio(err, tol))
    note = ":bit_equal" if bit_equal else ":rounded"
    r_la = rec(f"modes:{tag}:log_acc", err_la, LOG_ACC_TOL)
    r_e = rec(f"modes:{tag}:energy{note}", de, tol_e)
    r_f = rec(f"modes:{tag}:fitness{note}", df, tol_f)
    assert r_la <= 1.0, f"{tag}: log_acc differs by {float(np.max(err_la)):.3e} ({r_la:.2f} of the tolerance)"
    assert r_e <= 1.0, f"{tag}: energy history differs ({r_e:.2f} of the tolerance)"
    assert r_f <= 1.0, f"{tag}: fitness history differs ({r_f:.2f} of the tolerance)"
    assert np.array_equal(res["best_idx"][same], ref["best_idx"].numpy()[same]), f"{tag}: best states differ"
    if same[0] and res.get("random_traj") is not None:
        assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy()), f"{tag}: random_traj differs"
    if dev.get("temp") is not None:
        tp = dev["temp"]
        ens = same.reshape(-1, R).all(1)
        assert np.array_equal(tp["hist"][:, same], ref["rung_history"][:, same]), f"{tag}: rung history differs"
        assert np.array_equal(tp["rung"][same], ref["rung"][same]) and np.array_equal(tp["beta"][same], ref["beta"][same]), f"{tag}: final rungs differ"
        assert np.array_equal(tp["swap_attempts"][ens], ref["swap_attempts"][ens]), f"{tag}: swap attempts differ"
        assert np.array_equal(tp["swap_accepts"][ens], ref["swap_accepts"][ens]), f"{tag}: swap accepts differ"
    parted = sorted({nt[0] for nt in notes})
    return dict(parted=parted, notes=notes, log_acc=r_la, energy=r_e, fitness=r_f, bit_equal=bit_equal)


# ------------------------------------------------------------------------------------------------ planted faults (reference side)
class FaultyEnergy:
    """An energy with one planted fault of the chain-kernel glue, over `model` (anything DeviceEnergy takes):
      no_tf_in_accept     the transformer term is missing from the energy the accept ratio reads;
      fit_grad_flipped    the proposal rows hold lamda * d fit / dx although `which` has no bit 3 -- or lack it although it has;
      e_x_from_proposal   e_x is read from the proposal's slot (so e_y - e_x = 0)."""

    def __init__(self, model, which, kind):
        self.base, self.kind = DeviceEnergy(model, which), kind
        self.tf = DeviceEnergy(model, 4)
        self.other = DeviceEnergy(model, which ^ 8)
        self.pending = None

    def energy(self, idx):
        return self.base.energy(idx)                                         # the histories' first row is no part of the fault

    def energy_grad(self, idx):
        e, fit, g = self.base.energy_grad(idx)
        if self.kind == "no_tf_in_accept":
            e = e - self.tf.energy(idx)[0]
        elif self.kind == "fit_grad_flipped":
            g = self.other.energy_grad(idx)[2]
        elif self.kind == "e_x_from_proposal":
            # calls alternate x, y within an iteration: the x call's tensor is overwritten when y's energy is known, before the
            # iteration reads it
            if self.pending is None:
                self.pending = e
            else:
                self.pending.copy_(e)
                self.pending = None
        else:
            raise ValueError(self.kind)
        return e, fit, g


@contextlib.contextmanager
def beta_on_rows_only():
    """Inside the block helpers_tempering scales the gradient (the rows) by beta but leaves e_y - e_x unscaled."""
    orig = ht.ScaledEnergy

    class RowsOnly(orig):
        def energy_grad(self, idx):
            e, f, g = self.energy_fn.energy_grad(idx)
            self.raw.append((e, f))
            return e, f, self.beta.reshape(-1, 1, 1) * g

    ht.ScaledEnergy = RowsOnly
    try:
        yield
    finally:
        ht.ScaledEnergy = orig


@contextlib.contextmanager
def swap_on_scaled_energy(lamda):
    """Inside the block the swap rule reads lamda * E (for which = 2: fit * lamda instead of fit)."""
    orig = ht.swap_decision
    ht.swap_decision = lambda b_lo, b_hi, e_a, e_b, u: orig(b_lo, b_hi, np.float32(lamda) * np.float32(e_a), np.float32(lamda) * np.float32(e_b), u)
    try:
        yield
    finally:
        ht.swap_decision = orig


def population_law(K, start, T_):
    v = np.zeros(K.shape[0])
    v[start] = 1.0
    for _ in range(T_):
        v = v @ K
    return v


# ------------------------------------------------------------------------------------------------ the law cases
LAW_SITE = 10                      # one open residue of the toy model, inside the Potts window (4..19)
LAW_LETTERS_2 = 8                  # letters of the which = 2 ladder case
LAW_GAIN_2 = 256.0                 # ... whose CNNs' output layer is scaled by this (scaled_cnn): fitness spans 1.4 over the 8 states


def law_start_2(E):
    """Joint start state (rung 0, rung 1) of the ladder case: the states of lowest and highest energy, so that the first swap event
    decides something (from equal states d = 0: tests/test_tempering_cpu.py)."""
    return int(np.argmin(E)), int(np.argmax(E))


def kernels_of(energy, case, betas, pas):
    """helpers_tempering.kernels_of on a given energy: (Ks, states, index, E fp64 [S] untempered, inside)."""
    Ks, out = [], None
    for b in np.asarray(betas, dtype=np.float32):
        K, states, index, _, inside = hr.exact_reversible_kernel(ht.ScaledEnergy(energy, float(b)), case["wt"], case["allowed"], pas, 0,
                                                                 case["L"] - 1, case.get("nmut", 0))
        Ks.append(K)
        out = (states, index, inside)
    e32, _ = energy.energy(out[0])
    return Ks, out[0], out[1], e32.double().numpy(), out[2]

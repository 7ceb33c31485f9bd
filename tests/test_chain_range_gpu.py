"""The device-RNG chain kernels across the gradient's dynamic range (ppde_amd/csrc/pas.h: propose_body_dev, reverse_rows_dev, the
fused launch's own mref). They take exp(z - mref) against a fixed reference mref = min(beta spread / 2, 64) instead of reducing a
maximum per sub-step, so they are the only kernels here whose correctness depends on the magnitude of the gradient; the committed
fixtures reach a spread of 24 (tests/test_chain_range_cpu.py prints them). The matrix is tests/helpers_range.CELLS: Potts-only models
(which = 1) with planted fields, 32 chains, T = 12, pas_length 3, eager launches, traced.

Every cell that the CPU classification (helpers_range.expected: the numpy float32 restatement of the kernels' rows on the CPU oracle's
path, never device output) says runs is held to: both evaluation policies give identical arrays; draws, accept bits, best states,
random_traj (with a ladder: rung history and swap counters) equal to the fp32 reference on helpers_modes.DeviceEnergy and the device's
own noise, a chain parting only at a near-tie of the reference's own decision (race gap <= 1e-5, |log_acc - log u| <= 2e-4; at most one
chain or ensemble per cell and two cells in the module); energy histories within 2e-5 max(1, |e|); log_acc against helpers_range.score64
-- the reference's iteration functions in fp64 on the DEVICE's own path -- under the outer bound 2e-4 + 2^-23 (|e_y - e_x| + |log_acc|)
and the inner bound 4 x max(the cell's two yardsticks) + 16 x 2^-23 per sub-step. Every cell the classification says
meets a forward row whose normaliser is below 2^-125 or non-finite must end in ValueError (PPDE_ERR_NUMERIC) at sync().

Capped forward rows (a chain at the mutation cap, or a start state outside a reverts-only library: the two reverts are the only
admissible moves, their logits 5 apart, the better one `depth` below mref): depths -40 and -80 run and agree; -86 runs until an accepted
revert and a third mutation leave the second planted revert, at -91, as the best move; -95 and -110 are flagged. Before the guard on
S1 was moved from 0 to 2^-125 the -95 cells drew the two reverts about evenly where the reference draws the better one 99.3 % of the
time, recorded log((1 - 2^-23) / S3) for either, and flagged nothing (1 / S1 = inf for a denormal S1: every admissible entry became
1 - 2^-23); -110 (S1 = 0) was flagged then as now. The device's expf does return denormals: the window exists on the hardware.
Past the overflow edge (within, spread 320: z - mref = 96) the run ends in ValueError.

Reverse rows whose large spread is in g_y only (planted couplings, helpers_range.capped_reverse_model / gy_overflow_model).
Reversible mode, the reverse row of a path's first sub-step capped under a reference of 64 (DESIGN.md 4.2b's limit): depth -80 runs
and agrees; -95 (S1 denormal, 1 / S1 = inf) and -110 (S1 = 0 by underflow, told from a row without admissible entries by a bit
reduced next to the sums) reject the path and end in ValueError; before, both were rejected silently where the reference accepts
some of these paths. Default mode, one iteration, a reverse row with a logit 101.6 above mref: read first -- reverse_rows_dev had no
guard outside REV, S1 = inf gives inv = 0, every clamped entry 2^-23, logp_rev = log(1 / (20 L)) -- then run once on the parent
build: no error, a silently different log_acc. Now !(S1 < inf) is flagged there: ValueError."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_modes as hm
import helpers_range as R
from helpers import device_noise
from ppde_amd import library as dl
from test_hip_parity import observed

RESULT_KEYS = ("energy_history", "fitness_history", "best_idx", "best_energy", "best_fitness", "best_step", "random_traj")
TRACE_KEYS = ("flat", "accepted", "log_acc", "U")
PARTED_CELLS = []
RUNS = [c["name"] for c in R.CELLS if c["name"] not in R.FLAGGED]
FLAGS = [c["name"] for c in R.CELLS if c["name"] in R.FLAGGED]


@pytest.fixture(scope="module")
def models():
    from ppde_amd.energy import HipModel
    made = {}

    def get(c):
        key = c["model"]
        if key not in made:
            m = R.cell_model(c)
            hm_ = HipModel(m["wt"], "cuda:0")
            hm_.set_potts(m["J"], m["h"], m["i0"])
            hm_.set_lamda(0.0)
            made[key] = hm_
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _chains(c, model, reuse, trace=True):
    from ppde_amd.sampler import Chains
    m, lib, x0, nmut = R.cell_setup(c)
    ch = Chains(model, R.N, c["T"], R.PAS, nmut, False, m["lo"], m["hi"], 1, c["rng_mode"], reuse_grad=reuse, trace=trace, random_chain=0,
                use_graph=False, seed=c["seed"])
    if lib is not None:
        ch.set_library(lib)
    if c["mode"] != "default":
        ch.set_reversible(True)
    if c["betas"]:
        ch.set_tempering(c["betas"], 1)
    ch.init(torch.as_tensor(x0.astype(np.uint8)).cuda())
    return ch


def _run(c, model, reuse, trace=True, noise=None):
    """One run of the cell to its end; returns (dict(tr, res, temp), the noise the device drew). ValueError from sync() passes through."""
    ch = _chains(c, model, reuse, trace)
    try:
        if c["rng_mode"] == 0:
            for U, q, u in noise:
                ch.run(1, (U.to(torch.int32).reshape(1, -1), q.contiguous(), u.reshape(1, -1), [int(q.shape[0])]))
        else:
            ch.run(c["T"])
        ch.sync()
        if noise is None:
            noise = device_noise(ch, c["T"], R.PAS)
        temp = None
        if c["betas"]:
            st = ch.tempering_state()
            temp = dict(hist=ch.tempering_history(), rung=st["rung"], beta=st["beta"], swap_attempts=st["swap_attempts"],
                        swap_accepts=st["swap_accepts"])
        return dict(tr=ch.trace() if trace else None, res=ch.collect(), temp=temp), noise
    finally:
        ch.close()


def _same_bits(a, b, label, trace=True):
    for k in RESULT_KEYS:
        assert np.array_equal(a["res"][k], b["res"][k]), (label, k)
    if trace:
        for k in TRACE_KEYS:
            assert np.array_equal(a["tr"][k], b["tr"][k]), (label, k)
    if a["temp"] is not None:
        for k in a["temp"]:
            assert np.array_equal(a["temp"][k], b["temp"][k]), (label, k)


@pytest.mark.parametrize("name", RUNS)
def test_cell_runs_and_agrees(models, name):
    c = R.CELL[name]
    assert R.expected(c) == "runs"
    model = models(c)
    m, lib, _, _ = R.cell_setup(c)
    noise = R.cell_noise(c, m) if c["rng_mode"] == 0 else None
    runs = []
    for reuse in c["policies"]:
        dev, noise = _run(c, model, reuse, noise=noise)
        runs.append(dev)
    if len(runs) > 1:
        _same_bits(runs[0], runs[1], f"{name}: re-evaluate against reuse")
    if c["notrace"]:                                                           # the specialised kernels: no trace buffers
        for i, reuse in enumerate(c["policies"]):
            bare, _ = _run(c, model, reuse, trace=False)
            _same_bits(runs[i], bare, f"{name}: reuse {reuse} without trace", trace=False)
    dev = runs[0]
    tr, res = dev["tr"], dev["res"]
    en = hm.DeviceEnergy(model, 1)
    ref = R.reference_run(c, en, noise)
    Rg = len(c["betas"]) if c["betas"] else 1
    assert np.array_equal(tr["U"], np.stack([nz[0].numpy() for nz in noise])), f"{name}: path lengths differ"
    same, notes = hm.near_ties(tr, ref, noise, Rg)
    for note in notes:
        print(f"[range] {name}: chain {note[0]} parted at iteration {note[1]} ({note[2]}), margin {note[3]:.3e}")
    groups = {nt[0] // Rg for nt in notes}
    assert len(groups) <= 1, f"{name}: more than one chain (ensemble) left the reference: {notes}"
    if groups:
        PARTED_CELLS.append(name)
    assert len(PARTED_CELLS) <= 2, f"cells with a parted chain: {PARTED_CELLS}"
    if lib is not None:
        ok = dl.as_bool(lib).reshape(-1)
        for t in range(c["T"]):
            U = noise[t][0].numpy()
            for s in range(int(U.max())):
                assert ok[tr["flat"][t, s][s < U]].all(), f"{name}: a forbidden move was drawn"
    eh = ref["energy_history"].numpy()[:, same]
    r_e = observed(f"range:{name}:energy", np.abs(res["energy_history"][:, same] - eh), hm.E_TOL * np.maximum(1.0, np.abs(eh)))
    assert r_e <= 1.0, f"{name}: energy history differs ({r_e:.2f} of the tolerance)"
    assert np.array_equal(res["best_idx"][same], ref["best_idx"].numpy()[same]), f"{name}: best states differ"
    if same[0]:
        assert np.array_equal(res["random_traj"], ref["states"][:, 0].numpy()), f"{name}: random_traj differs"
    if dev["temp"] is not None:
        tp, ens = dev["temp"], same.reshape(-1, Rg).all(1)
        assert np.array_equal(tp["hist"][:, same], ref["rung_history"][:, same]), f"{name}: rung history differs"
        assert np.array_equal(tp["swap_attempts"][ens], ref["swap_attempts"][ens]) and np.array_equal(tp["swap_accepts"][ens], ref["swap_accepts"][ens])
    # log_acc on the device's OWN path (every chain, parted or not) against the fp64 score of that path
    path = dict(flat=tr["flat"], U=tr["U"], accepted=tr["accepted"], rung_history=None if dev["temp"] is None else dev["temp"]["hist"])
    s64 = R.score64(c, en, path)
    assert not s64["mismatch"].any(), f"{name}: the device accepted a path the mode's rule refuses"
    y1 = float(R.log_acc_error(R.score(c, en, path, torch.float32)["log_acc"], s64["log_acc"]).max())
    y2 = float(R.log_acc_error(R.score(c, en, path, torch.float32, emulate=True)["log_acc"], s64["log_acc"]).max())
    err = R.log_acc_error(tr["log_acc"], s64["log_acc"])
    r_out = observed(f"range:{name}:log_acc:outer", err, R.outer_bound(s64["log_acc"], s64["de"]))
    r_in = observed(f"range:{name}:log_acc:inner", err, R.inner_bound((y1, y2), tr["U"]))
    print(f"[range] {name}: yardsticks fp32 oracle {y1:.3e}, fixed-reference fp32 {y2:.3e}; device log_acc off by {err.max():.3e} = {r_out:.3f} of the "
          f"outer, {r_in:.3f} of the inner bound; largest |e_y - e_x| {np.abs(s64['de']).max():.1f}; accepted {tr['accepted'].mean():.2f}")
    assert r_out <= 1.0, f"{name}: log_acc differs from the fp64 score by {err.max():.3e} ({r_out:.2f} of the outer bound)"
    assert r_in <= 1.0, f"{name}: log_acc differs from the fp64 score by {err.max():.3e} ({r_in:.2f} of the inner bound)"


@pytest.mark.parametrize("name", FLAGS)
def test_cell_ends_in_value_error(models, name):
    """A forward row whose normaliser underflows (or overflows) against the fixed reference: PPDE_ERR_NUMERIC at sync(), whichever
    policy runs it -- never a silently different trajectory. The reference itself carries on in the capped cells (it reduces a maximum
    per row)."""
    c = R.CELL[name]
    assert R.expected(c) == "flag"
    for reuse in c["policies"]:
        with pytest.raises(ValueError, match="no usable mass"):             # PPDE_ERR_NUMERIC's message, no other ValueError
            _run(c, models(c), reuse)

"""The dynamic-range matrix of the device-RNG chain kernels on the CPU (tests/helpers_range.py; the GPU side is
tests/test_chain_range_gpu.py): what regime every GPU cell is in, what the two yardsticks of its log_acc are, that the reference
alone meets no near-tie in any cell, and that each planted fault of the fixed-reference arithmetic is rejected in a named cell.

Everything here runs the reference (oracle/ppde_oracle.py and the mode helpers) on the CPU Potts oracle and on the device RNG's draws
restated on the CPU (orc.device_noise); the device's arithmetic is the numpy float32 restatement helpers_range.fixed_reference_fp32.
A cell's expected behaviour on the GPU (runs and agrees / PPDE_ERR_NUMERIC) is derived HERE, from the class of every forward row's
normaliser along the fp32 oracle's path, never from device output. Run with -s for the tables DESIGN.md 4.2 and 5 quote."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import helpers_modes as hm
import helpers_range as R
from helpers import GOLDEN, compare_runs_up_to_near_ties

# the cells whose forward rows leave the normal class somewhere along the path, and the class they reach. capped:default:-86 starts
# normal (depth -86) and reaches the window once its first revert is accepted and a third mutation puts it back on the cap: the
# second planted revert, 5 below the first, is then the best admissible move at depth -91. All of them end in PPDE_ERR_NUMERIC.
ABNORMAL = {"capped:default:-86": ("fwd", "recip_inf"), "capped:default:-95": ("fwd", "recip_inf"), "capped:lib:-95": ("fwd", "recip_inf"),
            "capped:default:-110": ("fwd", "zero"), "capped:lib:-110": ("fwd", "zero"), "overflow:within:320": ("fwd", "inf"),
            "revcap:-95": ("rev", "recip_inf"), "revcap:-110": ("rev", "zero"), "overflow:gy_only:330": ("rev", "inf")}
EXPECT_FLAG = ABNORMAL
# fault -> the cell that must reject it, and how
FAULT_CELLS = {"mref_uncapped": "capped:default:-40", "mref_without_beta": "modes:ladder_steep:within:96", "S1_carried": "sweep:L24:within:200",
               "reverse_mref_over_range": "outside:within:240", "unguarded_window": "capped:default:-95"}


@functools.lru_cache(maxsize=None)
def _cell(name):
    """Reference run, its trace, fp64 / fp32 / emulated scores on the reference's path and the emulation's row log of one cell."""
    c = R.CELL[name]
    m = R.cell_model(c)
    en = R.oracle_energy(m)
    noise = R.cell_noise(c, m)
    ref = R.reference_run(c, en, noise)
    tr = R.as_trace(ref, noise)
    s64 = R.score64(c, en, tr)
    s32 = R.score(c, en, tr, torch.float32)
    log, emu, flag = [], None, None
    try:
        with R.emulated(c, log=log) as wrap:
            emu = R.reference_run(c, R.emulated_energy(c, en, wrap), noise, emulate=True)
    except R.NumericFlag as e:
        flag = str(e)
    y2 = None
    if flag is None:
        se = R.score(c, en, tr, torch.float32, emulate=True)
        y2 = float(R.log_acc_error(se["log_acc"], s64["log_acc"]).max())
    y1 = float(R.log_acc_error(s32["log_acc"], s64["log_acc"]).max())
    return dict(c=c, m=m, en=en, noise=noise, ref=ref, tr=tr, s64=s64, s32=s32, log=log, emu=emu, flag=flag, y1=y1, y2=y2)


def _classes(log, phase):
    out = {}
    for ph, cls, _, _ in log:
        if ph == phase:
            for k in cls.tolist():
                out[k] = out.get(k, 0) + 1
    return out


@pytest.mark.parametrize("name", [c["name"] for c in R.CELLS])
def test_regime_of_every_gpu_cell(name):
    """The realised spread, mref and its side of the cap, the largest z - mref and the class of every row's S1 along the path."""
    r = _cell(name)
    c, m = r["c"], r["m"]
    key = c["model"]
    beta0 = max(c["betas"]) if c["betas"] else 1.0
    mref = min(beta0 * m["spread"] / 2.0, R.MREF_CAP)
    top = max(float(np.max(d)) for ph, _, _, d in r["log"] if ph == "fwd")
    fwd, rev = _classes(r["log"], "fwd"), _classes(r["log"], "rev")
    print(f"[range] {name}: spread {m['spread']:.3f}, mref(beta {beta0:g}) {mref:.3f} ({'capped at 64' if beta0 * m['spread'] / 2 >= 64 else 'follows the spread'}), "
          f"largest forward z - mref {top:.3f}, depth {m.get('depth')}, forward rows {fwd}, reverse rows {rev}, "
          f"emulation: {'flags PPDE_ERR_NUMERIC' if r['flag'] else 'runs'}")
    if key[0] == "spread" and key[2] != "tiny":
        assert abs(m["spread"] - key[2]) < 1e-3
        assert (m["spread"] / 2 >= 64) == (key[2] >= 128)                       # 127 follows the spread, 129 sits on the cap
        if key[3] == "within" and name not in EXPECT_FLAG and not c["betas"]:
            assert abs(top - (beta0 * key[2] / 2 - mref)) < 1e-3                 # one residue carries the spread: z reaches spread / 2
            assert top < 88.7
        if key[3] == "across" and not c["betas"]:
            assert top <= beta0 * (key[2] / 8 + 3.0) - mref                      # no logit follows the reference (3: the unplanted couplings' own)
    if key[0] == "spread" and key[2] == "tiny":
        assert m["spread"] < 1e-3 and abs(top) < 1e-3
    if key[0] == "capped":
        assert abs(m["depth"] - key[1]) < 0.05 and abs(m["revert_gap"] - 5.0 * key[2]) < 1e-3 and abs(mref - (64.0 if key[2] == 1.0 else 50.0)) < 0.05
        first = r["log"][0]
        assert first[0] == "fwd" and abs(float(first[3].min()) - m["depth"]) < 1e-3   # the first row of every chain (rung 0's) is the capped one
    if key[0] == "outside":
        assert m["spread"] < 128 and m["spread_all"] >= key[2] - 1e-3
    odd = {(ph, k) for ph, seen in (("fwd", fwd), ("rev", rev)) for k in seen if k != "normal"}
    assert odd == ({ABNORMAL[name]} if name in ABNORMAL else set()), odd
    if key[0] == "revcap":                                                     # the capped reverse row is reached, at the planted depth
        seen = np.concatenate([d for ph, _, _, d in r["log"] if ph == "rev"])
        assert np.isclose(seen, m["depth"], atol=1e-3).any() and abs(m["depth"] - key[1]) < 0.05 and abs(m["revert_gap"] - 5.0) < 1e-3
        # (a path of ONE move ends on the capped state itself and is refused for the cap; its reverse row holds only the worse revert)
        assert abs(float(seen.min()) - (m["depth"] - 5.0)) < 1e-3
        assert m["spread_y"] >= 200 and m["spread_y"] - m["spread"] > 150        # g_y's spread, not g_x's, is the large one
    if key[0] == "gy_overflow":
        assert m["spread"] < 128 and m["spread_y"] > 2 * (64 + 88.7) and m["top_y"] > 88.7
    if name in EXPECT_FLAG:
        assert r["flag"] is not None and name in R.FLAGGED
    else:
        assert r["flag"] is None and set(rev) == {"normal"}, (r["flag"], fwd, rev)
        # the emulation draws and decides what the reference does (another rounding of the same arithmetic) -- up to near-ties
        dev = hm.as_device_run(r["emu"], r["noise"], 2 * R.PAS - 1)
        _, notes = hm.near_ties(dev["tr"], r["ref"], r["noise"], len(c["betas"]) if c["betas"] else 1)
        assert len({n[0] for n in notes}) <= 1, notes


def test_expected_behaviour_covers_the_matrix():
    """Which cells the GPU module expects to end in PPDE_ERR_NUMERIC: exactly the ones whose forward rows leave the normal class."""
    assert {c["name"] for c in R.CELLS if R.expected(c) == "flag"} == set(EXPECT_FLAG) == set(R.FLAGGED)


def test_yardsticks_of_every_cell():
    """max |log_acc(fp32 oracle) - log_acc(fp64)| and the same for the fixed_reference_fp32 evaluation, on the reference's own path."""
    worst = 0.0
    for c in R.CELLS:
        r = _cell(c["name"])
        assert not r["s64"]["mismatch"].any() and not r["s32"]["mismatch"].any()
        bound = R.outer_bound(r["s64"]["log_acc"], r["s64"]["de"])
        print(f"[range] yardsticks {c['name']}: fp32 oracle {r['y1']:.3e}, fixed-reference fp32 {'flagged' if r['y2'] is None else format(r['y2'], '.3e')}, "
              f"largest |e_y - e_x| {np.abs(r['s64']['de']).max():.1f}, outer bound up to {bound.max():.3e}")
        # the reference's own fp32 evaluation sits inside the outer bound it is used with
        assert (R.log_acc_error(r["s32"]["log_acc"], r["s64"]["log_acc"]) <= bound).all()
        if r["y2"] is not None:
            worst = max(worst, r["y2"])
            assert r["y2"] <= bound.max()
    print(f"[range] largest fixed-reference yardstick {worst:.3e}")


def test_the_reference_alone_parts_no_chain():
    """No decision of the reference comes within the near-tie thresholds in any cell: a parted chain on the GPU is the device's doing."""
    for c in R.CELLS:
        if c["name"] in EXPECT_FLAG:
            continue                                                           # (nothing of such a run is compared on the GPU)
        r = _cell(c["name"])
        acc_margin, gap = hm.margins(r["noise"], r["ref"])
        print(f"[range] margins {c['name']}: |log_acc - log u| >= {acc_margin:.3e}, race gap >= {gap:.3e}")
        assert acc_margin > R.ACC_TOL and gap > R.GAP_TOL, (c["name"], acc_margin, gap)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_is_rejected(fault):
    """The emulated run with the fault against the reference of the named cell: a draw or an accept bit that is no near-tie, a log_acc
    beyond the outer bound, or "flag": the faulty arithmetic loses a row's mass (NumericFlag) in a cell whose unfaulted emulation
    runs to the end. On the device that is PPDE_ERR_NUMERIC, a ValueError at sync(), in a cell tests/test_chain_range_gpu.py requires
    to run and agree: the cell fails there as it does for a wrong draw. Three faults leave by that channel: against a softmax
    reference that is too large or a cancelled sum the guard on S1 speaks before any draw can differ."""
    name = FAULT_CELLS[fault]
    r = _cell(name)
    c = r["c"]
    how = None
    try:
        with R.emulated(c, fault=fault) as wrap:
            bad = R.reference_run(c, R.emulated_energy(c, r["en"], wrap), r["noise"], emulate=True)
    except R.NumericFlag:
        how = "flag"
        assert r["flag"] is None, "the cell flags without the fault too"
    if how is None:
        dev = hm.as_device_run(bad, r["noise"], 2 * R.PAS - 1)
        notes = None
        try:                                                                   # (the helper raises only on a difference that is no near-tie)
            _, notes, _ = compare_runs_up_to_near_ties(dev["tr"], r["ref"], r["noise"], R.GAP_TOL, R.ACC_TOL)
        except AssertionError:
            how = "draw or accept bit"
        if how is None:
            assert not notes, f"{fault} in {name}: classed as a near-tie {notes}"
            err = R.log_acc_error(dev["tr"]["log_acc"], np.stack([o["log_acc"].numpy() for o in r["ref"]["traces"]]))
            if (err > R.outer_bound(r["s64"]["log_acc"], r["s64"]["de"])).any():
                how = "log_acc"
    print(f"[range] fault {fault}: rejected in {name} by {how}")
    assert how is not None, f"{fault} passes in {name}"
    if fault == "unguarded_window":
        assert how == "draw or accept bit"                                     # the predicted bug: half the draws go to the worse revert


def test_spreads_of_the_committed_fixtures():
    """What has been run so far: the row spread (max - min over the proposal range) of every committed fixture gradient."""
    seen = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        fx = np.load(path, allow_pickle=False)
        for key in ("grad", "t_grad", "pt_grad"):
            if key in fx.files and fx[key].ndim >= 3 and fx[key].shape[-1] == 20:
                g = fx[key].reshape(-1, fx[key].shape[-2], 20)
                lo, hi = 0, g.shape[1] - 1
                if "win_start" in fx.files and "Lp" in fx.files:
                    lo, hi = int(fx["win_start"]), int(fx["win_start"]) + int(fx["Lp"]) - 1
                sp = g[:, lo:hi + 1].reshape(g.shape[0], -1)
                sp = sp.max(1) - sp.min(1)
                seen.append(float(sp.max()))
                print(f"[range] fixture {os.path.basename(path)}[{key}]: spread {sp.min():.2f} .. {sp.max():.2f} over {g.shape[0]} rows")
    assert seen and max(seen) < 64, "a committed fixture reaches the matrix's range: say so in DESIGN.md 4.2"

"""The transformer expert on the device across the dynamic range of its weights (tests/helpers_tf_range.py), against fp64.

Every case rescales make_esm2_state's weights -- the residual stream, q against k, v against out_proj, the layer-norm gains
against the matrices behind them (function-preserving, run at BOTH edges of the range tests/test_transformer_range_cpu.py
computes), or peaked attention, logits in the tens and one dominant stream channel (run at the largest exponent at which the
bounds still reject what they reject at unit scale) -- and applies check_stages of tests/test_transformer_stages_gpu.py
unchanged: every teacher-forced stage A .. G and the whole-model bounds, MARGIN x the yardstick measured on the case's own
weights, pad columns exactly zero, no row, head, chain or stage exempt. Inside a supported range the whole-model yardsticks are
also required to be the ones the CPU module admitted (within 2 x their unit-scale values), so that no bound widens unnoticed.
Ratios: test_hip_parity.observed, tfrange:<geometry>:<family><exponent>:<stage>.

Then: weights the device cannot hold or evaluate are refused by ppde_model_set_transformer with the expert that was there
left answering bit for bit, and a chain that goes non-finite leaves its batch neighbours' bits alone."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_tf_range as hr
import helpers_transformer as ht
from ppde_amd import _hip
from test_transformer_stages_gpu import REPO, check_stages, device_buffers


def _tag(geom, family, exponent, layers, suffix=""):
    return f"{geom}{'' if layers == 2 else 'l1'}:{family}{exponent}{suffix}"


def _case(geom, family, exponent, layers, raw=None, suffix=""):
    L, dim, heads, ffn, n = hr.GEOMS[geom]
    st = hr.regime(hr.state(geom, layers), family, exponent, layers)
    print(f"[tfrange] {geom} ({L} residues, width {dim}, {heads} heads, {layers} layers, {n} chains): {family} x 2^{exponent}{suffix}", flush=True)
    if raw is None:
        raw = device_buffers(L, layers, dim, heads, ffn, n, state=st)
    check_stages(_tag(geom, family, exponent, layers, suffix), L, layers, dim, heads, ffn, raw, stages=layers == 2, family="tfrange", state=st)


@pytest.mark.parametrize("geom,family,exponent", hr.CASES, ids=[f"{g}-{f}{e}" for g, f, e in hr.CASES])
def test_every_stage_and_the_whole_model_backward_across_the_range(geom, family, exponent):
    if family in hr.RANGE:
        # the bound is MARGIN x a yardstick no larger than the CPU module admitted: that one (host-independent) within 2 x its
        # unit-scale value, and check_stages' own, another draw of the same rounding process, within 2 x that one
        assert hr.rows_admitted(geom, family, exponent)
        y, own = hr.case_yardsticks(geom, 2, family, exponent), hr.case_yardsticks(geom, 2, family, exponent, ht.F32)
        assert own is not None and all(own[k] <= 2.0 * y[k] for k in hr.ROW_YARDSTICKS), (own, y)
    _case(geom, family, exponent, 2)
    _case(geom, family, exponent, 1)


#            variable          suffix     cases
ALT_FORMS = {"PPDE_TF_ATT_KO": ("+ko=0", [(g, "sharp", hr.PEAKED["sharp"]) for g in ("17x128", "129x256", "237x96")]),      # the multi-pass tf_attn_bwd
             "PPDE_TF_LN16": ("+ln16=0", [(g, "stream", e) for g in ("17x128", "129x256") for e in hr.RANGE["stream"]])}    # one row per wavefront

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np
import helpers_tf_range as hr
from test_transformer_range_gpu import ALT_FORMS
from test_transformer_stages_gpu import device_buffers
out = {}
for geom, family, exponent in ALT_FORMS[sys.argv[3]][1]:
    L, dim, heads, ffn, n = hr.GEOMS[geom]
    for layers in (2, 1):
        st = hr.regime(hr.state(geom, layers), family, exponent, layers)
        for k, v in device_buffers(L, layers, dim, heads, ffn, n, state=st).items():
            out[f"{geom}/{family}/{exponent}/{layers}/{k}"] = v
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("var", sorted(ALT_FORMS))
def test_alternative_kernel_forms_across_the_range(var):
    """Both variables are read once per process: a fresh child writes the buffers, the same checks run here."""
    suffix, cases = ALT_FORMS[var]
    with tempfile.TemporaryDirectory() as d:
        script, out = os.path.join(d, "child.py"), os.path.join(d, "buffers.npz")
        open(script, "w").write(_CHILD)
        r = subprocess.run([sys.executable, script, REPO, out, var], capture_output=True, text=True, timeout=300, env=dict(os.environ, **{var: "0"}))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got = dict(np.load(out))
    for geom, family, exponent in cases:
        for layers in (2, 1):
            pre = f"{geom}/{family}/{exponent}/{layers}/"
            _case(geom, family, exponent, layers, raw={k[len(pre):]: v for k, v in got.items() if k.startswith(pre)}, suffix=suffix)


# ---- past the edge, refusals, isolation ------------------------------------------------------------------------------------
def _new_model(geom, state=None, layers=2):
    from test_transformer_gpu import _model
    L, dim, heads, ffn, n = hr.GEOMS[geom]
    return _model(L, layers, dim, heads, ffn, state=state)[0]


def _eval(m, idx):
    e, _, g = m.energy_grad(torch.as_tensor(idx).cuda(), 4)
    return e.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("geom,family", [("17x128", "stream"), ("17x128", "lngain"), ("24x768", "stream"), ("24x768", "lngain")])
def test_one_step_past_the_finite_range_no_finite_number_is_accepted(geom, family):
    """Where the half-points evaluation is no longer finite (an fp16 activation beyond 65504), the device either refuses the
    model -- the wild type's score is not finite -- or returns non-finite energies for every chain the CPU evaluation loses."""
    L, dim, heads, ffn, n = hr.GEOMS[geom]
    e = hr.OVERFLOW[family]
    st = hr.regime(hr.state(geom, 2), family, e, 2)
    _, idx, _, half = hr.evaluate(geom, 2, family, e)
    lost = ~np.isfinite(half["score"].numpy())
    assert lost.any()
    print(f"[tfrange] {geom}: {family} x 2^{e}, past the range; the half-points evaluation loses chains {np.flatnonzero(lost).tolist()}", flush=True)
    try:
        m = _new_model(geom, st)
    except ValueError as err:                                      # PPDE_ERR_NUMERIC
        assert "not finite" in str(err) and lost[0]                # refused on the wild type's account (chain 0 is the wild type)
        return
    got, _ = _eval(m, idx)
    m.close()
    assert not np.isfinite(got[lost]).any(), got


def test_weights_the_device_cannot_hold_or_evaluate_are_refused_and_the_expert_that_was_there_stays():
    geom = "17x128"
    L, dim, heads, ffn, n = hr.GEOMS[geom]
    st = hr.state(geom, 2)
    _, idx = ht.chains_like_the_parity_test(L, n)
    m = _new_model(geom)
    before = _eval(m, idx) + (m.transformer_wt_score,)

    def still_there():
        after = _eval(m, idx) + (m.transformer_wt_score,)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))

    # a matrix entry that is finite in fp32 and inf in fp16; a NaN bias; an inf gain: PPDE_ERR_INVALID naming tensor and layer
    for name, pos, value, says in (("layers.1.fc2.weight", (3, 5), 65520.0, "fc2.weight of layer 1"),
                                   ("layers.0.self_attn.k_proj.weight", (0, 0), -1e6, "k_proj.weight of layer 0"),
                                   ("embed_tokens.weight", (32, dim - 1), np.inf, "embed_tokens.weight"),
                                   ("layers.0.self_attn.q_proj.bias", (7,), np.nan, "q_proj.bias of layer 0"),
                                   ("lm_head.layer_norm.weight", (0,), np.inf, "lm_head.layer_norm.weight")):
        bad = {k: np.array(v, copy=True) for k, v in st.items()}
        bad[name][pos] = value
        with pytest.raises(_hip.PpdeHipError, match=r"\[-1\].*" + says.replace(".", r"\.")):
            m.set_transformer(bad, heads)
        still_there()
    ok = {k: np.array(v, copy=True) for k, v in st.items()}
    ok["layers.1.fc2.weight"][3, 5] = 65519.0                       # rounds to 65504: held, and accepted
    m2 = _new_model(geom, ok)
    assert np.isfinite(m2.transformer_wt_score)
    m2.close()
    # weights of finite entries on which the wild type's score is not finite: PPDE_ERR_NUMERIC, after the kernels have run
    with pytest.raises(ValueError, match="wild type's transformer score is not finite"):
        m.set_transformer(hr.regime(st, "stream", hr.OVERFLOW["stream"], 2), heads)
    still_there()
    m.set_transformer(hr.regime(st, "stream", 3, 2), heads)         # and a valid replacement still replaces
    assert not np.array_equal(_eval(m, idx)[1], before[1])
    m.close()


def test_a_non_finite_chain_leaves_its_batch_neighbours_bits_alone():
    geom, letter, victim = "17x128", 19, 3
    L, dim, heads, ffn, _ = hr.GEOMS[geom]
    wt, idx = ht.chains_like_the_parity_test(L, 5)
    assert not (idx == letter).any() and not (wt == letter).any()
    with_it = idx.copy()
    with_it[victim, 11] = letter
    st = hr.letter_overflow(hr.state(geom, 2), letter)
    # the CPU evaluation that rounds where the device rounds: that chain is lost, the others are not
    half = ht.model(ht.Params(st, 2, dim, heads), with_it, ht.F32, half=True, want_grad=False)["score"].numpy()
    others = [c for c in range(5) if c != victim]
    assert not np.isfinite(half[victim]) and np.isfinite(half[others]).all()
    m = _new_model(geom, st)
    assert np.isfinite(m.transformer_wt_score)
    e_all, g_all = _eval(m, with_it)
    e_ref, g_ref = _eval(m, idx[others])
    m.close()
    assert not np.isfinite(e_all[victim])
    assert np.isfinite(e_all[others]).all()
    assert np.array_equal(e_all[others], e_ref) and np.array_equal(g_all[others], g_ref, equal_nan=True)

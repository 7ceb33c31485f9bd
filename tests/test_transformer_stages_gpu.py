"""Every stage of the transformer expert on the device against fp64, bounded by a yardstick measured in the same test.

Each stage (tests/helpers_transformer.py: A .. G) is fed the DEVICE's own input, read back with
ppde_debug_transformer_read, so that one stage's error is not buried under the preceding layers'; its device output is
compared with the fp64 evaluation of that stage on that input. The bound is 4 x yardstick, the yardstick being the distance,
in the same measure and on the same input, between fp64 and the evaluation that rounds to fp16 where the device does. It is
computed on the CPU here and never from device output. What has no readable upstream gradient -- d logits through the head
and the layers to d embedding -- is checked on whole two- and one-layer models against fp64 autograd: d q|k|v of layer 0
(with one layer: the attention backward behind only the head and the feed-forward backward), d embedding, the gradient,
the score. Pad columns (dim .. padded dim, logits 33 .. 127) must be exactly zero. No row, head, chain or stage is exempt.
The ratios are recorded by test_hip_parity.observed under tfstage:<geometry>:<stage>[:layer];
tests/test_transformer_stages_cpu.py shows what the bounds reject."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_transformer as ht
from helpers_transformer import F32, F64
from ppde_amd import synthetic
from test_hip_parity import observed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        L   dim heads ffn  chains
GEOMS = [(17, 128, 4, 256, 3),        # two key tiles, one row in the tail tile
         (128, 128, 4, 256, 3),       # the 128-residue kernels, full
         (129, 128, 4, 256, 3),       # the 256-residue kernels, one row past 128
         (237, 256, 8, 512, 2),       # GFP length, pad keys in the last tile
         (129, 256, 4, 512, 2),       # head width 64 past 128
         (256, 128, 2, 256, 2),       # rows-only LDS image, the longest sequence
         (237, 96, 4, 256, 2),        # head width 24, rows padded 96 -> 128
         (104, 480, 20, 1920, 2),     # 35M widths, rows of 480 in 512
         (24, 768, 12, 1024, 3),      # tf_ln_bwd<2> behind tf_ln_fwd16<10>
         (24, 1536, 24, 1024, 3)]     # tf_ln_fwd<3> / tf_ln_bwd<3> at the widest row the ABI accepts
ALT_FORMS = [(129, 128, 4, 256, 3), (237, 96, 4, 256, 2)]     # run again under PPDE_TF_LN16=0 and under PPDE_TF_ATT_KO=0


def read_buffers(m, L, layers, dim, ffn, n):
    """Every activation buffer the checks read, after an evaluation of n chains with the gradient; pad columns included."""
    from test_transformer_gpu import _read
    dp = (dim + 127) // 128 * 128
    b = {}
    for i in range(layers):
        b[f"xin{i}"], b[f"qkv{i}"] = _read(m, 0, i, (n, L, dp)), _read(m, 1, i, (n, L, 3, dp))
        b[f"xmid{i}"], b[f"gp{i}"] = _read(m, 3, i, (n, L, dp)), _read(m, 4, i, (n, L, ffn))
    for name, what, shape in (("xlast", 5, (n, L, dp)), ("logits", 6, (n, L, 128)), ("dlogits", 7, (n, L, 128)), ("demb", 8, (n, L, dp)),
                              ("dtok", 9, (n, L, 128)), ("ctx", 10, (n, L, dp)), ("dqkv0", 11, (n, L, 3, dp))):
        b[name] = _read(m, what, 0, shape)
    return b


def device_buffers(L, layers, dim, heads, ffn, n, state=None):
    """One evaluation with the gradient on the device; every buffer the checks read, pad columns included. `state`: the weights,
    where they are not make_esm2_state(seed=3)."""
    from test_transformer_gpu import _model
    m, wt, _, _ = _model(L, layers, dim, heads, ffn, state=state)
    wt2, idx = ht.chains_like_the_parity_test(L, n)
    assert np.array_equal(wt, wt2)
    e, _, g = m.energy_grad(torch.as_tensor(idx).cuda(), 4)
    b = dict(idx=idx, e=e.cpu().numpy(), grad=g.cpu().numpy(), wt_score=np.float64(m.transformer_wt_score))
    b.update(read_buffers(m, L, layers, dim, ffn, n))
    m.close()
    return b


def _strip_pads(b, dim, layers):
    """Pad columns must be exactly zero; -> the buffers at the model's own widths, as tensors."""
    out = {}
    for k, v in b.items():
        if k in ("idx", "e", "grad", "wt_score") or k.startswith("gp"):
            out[k] = v
        elif k in ("logits", "dlogits", "dtok"):
            assert not v[..., 33:].any(), f"pad columns of {k}"
            out[k] = v[..., :33]
        else:
            assert not v[..., dim:].any(), f"pad columns of {k}"
            out[k] = v[..., :dim].reshape(v.shape[0], v.shape[1], -1)
    return {k: (torch.as_tensor(v) if k not in ("idx", "wt_score") else v) for k, v in out.items()}


def check_stages(tag, L, layers, dim, heads, ffn, raw, stages=True, chains=None, family="tfstage", state=None):
    """Apply every check to one device evaluation; the assertion comes last so that a failure reports all of its ratios.
    `chains`: check these chains of the evaluation only (every buffer, idx, e and grad sliced on the chain axis; the first
    one must be the wild type); within them no row, head or stage is exempt. `state`: the weights the device was given, where
    they are not make_esm2_state(seed=3); reference and yardstick are evaluated on them."""
    P = ht.Params(synthetic.make_esm2_state(layers, dim, heads, ffn, seed=3) if state is None else state, layers, dim, heads)
    if chains is not None:
        raw = {k: (v if k == "wt_score" else np.ascontiguousarray(np.asarray(v)[list(chains)])) for k, v in raw.items()}
    b = _strip_pads(raw, dim, layers)
    idx, D = b["idx"], dim
    ratios = {}

    def bound(name, measure, got, ref, half):
        yard = measure(half, ref)
        assert yard > 0, name
        ratios[name] = observed(f"{family}:{tag}:{name}", measure(got, ref), ht.MARGIN * yard)

    thirds = lambda f: (lambda a, r: max(f(a[..., j * D:(j + 1) * D], r[..., j * D:(j + 1) * D]) for j in range(3)))
    if stages:
        for i in range(layers):
            xin, qkv, xmid = b[f"xin{i}"], b[f"qkv{i}"], b[f"xmid{i}"]
            xout = b[f"xin{i + 1}"] if i + 1 < layers else b["xlast"]
            bound(f"A:{i}", thirds(ht.row_rel), qkv, ht.stage_a(P, i, xin, F64), ht.stage_a(P, i, xin, F32, True))
            bound(f"B:{i}", ht.row_rel, xmid, ht.stage_b(P, i, xin, qkv, F64)[1], ht.stage_b(P, i, xin, qkv, F32, True)[1])
            r, h = ht.stage_c(P, i, xmid, F64), ht.stage_c(P, i, xmid, F32, True)
            bound(f"C.gelu':{i}", ht.row_rel, b[f"gp{i}"], r[0], h[0])
            bound(f"C:{i}", ht.row_rel, xout, r[1], h[1])
        qkv = b[f"qkv{layers - 1}"]
        bound("B'", lambda a, r: ht.slice_rel(a, r, P.hd), b["ctx"], ht.attention(P, qkv, F64), ht.attention(P, qkv, F32, True))
        bound("D", ht.row_rel, b["logits"], ht.stage_d(P, b["xlast"], F64), ht.stage_d(P, b["xlast"], F32, True))
        wt_s = float(b["wt_score"])
        r, h = ht.stage_e(P, b["logits"], idx, F64, wt_score=wt_s), ht.stage_e(P, b["logits"], idx, F32, True, wt_score=wt_s)
        raw_s = ht.stage_e(P, b["logits"], idx, F64)[0]
        bound("E.score", lambda a, rr: ht.score_rel(a, rr, raw_s), b["e"], r[0], h[0])
        bound("E.dlogits", ht.row_rel, b["dlogits"], r[1], h[1])
        bound("F", ht.row_rel, b["dtok"], ht.stage_f(P, b["demb"], F64), ht.stage_f(P, b["demb"], F32, True))
        bound("G", ht.chain_rel, b["grad"], ht.stage_g(P, b["dtok"], b["logits"], F64), ht.stage_g(P, b["dtok"], b["logits"], F32, True))
    # the whole model under autograd: what no stage can be fed
    ref, half = ht.model(P, idx, F64), ht.model(P, idx, F32, half=True)
    bound("model.dqkv0", lambda a, r: ht.slice_rel(a, r, P.hd, 3), b["dqkv0"], ref["dqkv0"], half["dqkv0"])
    bound("model.demb", ht.chain_rel, b["demb"], ref["demb"], half["demb"])
    bound("model.grad", ht.chain_rel, b["grad"], ref["grad"], half["grad"])
    bound("model.score", ht.score_rel, b["e"].double() + float(b["wt_score"]), ref["score"], half["score"])
    assert float(b["e"][0]) == 0.0                                  # chain 0 is the wild type
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{tag}: device distance from fp64 over 4 x yardstick: {bad}"


def _tag(L, layers, dim, heads, suffix=""):
    return f"{L}x{dim}h{heads}l{layers}{suffix}"


@pytest.mark.parametrize("L,dim,heads,ffn,n", GEOMS, ids=[f"{g[0]}x{g[1]}h{g[2]}" for g in GEOMS])
def test_every_stage_and_the_whole_model_backward_vs_fp64(L, dim, heads, ffn, n):
    check_stages(_tag(L, 2, dim, heads), L, 2, dim, heads, ffn, device_buffers(L, 2, dim, heads, ffn, n))
    check_stages(_tag(L, 1, dim, heads), L, 1, dim, heads, ffn, device_buffers(L, 1, dim, heads, ffn, n), stages=False)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np
from test_transformer_stages_gpu import ALT_FORMS, device_buffers
out = {}
for L, dim, heads, ffn, n in ALT_FORMS:
    for layers in (2, 1):
        for k, v in device_buffers(L, layers, dim, heads, ffn, n).items():
            out[f"{L}/{layers}/{k}"] = v
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("var,suffix", [("PPDE_TF_LN16", "+ln16=0"), ("PPDE_TF_ATT_KO", "+ko=0")])
def test_alternative_kernel_forms_vs_fp64(var, suffix):
    """PPDE_TF_LN16=0: one row per wavefront (tf_ln_fwd<2> / tf_ln_bwd<2> at small widths); PPDE_TF_ATT_KO=0: the multi-pass
    tf_attn_bwd. Both are read once per process: a fresh child writes the buffers, the same checks run here."""
    with tempfile.TemporaryDirectory() as d:
        script, out = os.path.join(d, "child.py"), os.path.join(d, "buffers.npz")
        open(script, "w").write(_CHILD)
        r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=300, env=dict(os.environ, **{var: "0"}))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got = dict(np.load(out))
    for L, dim, heads, ffn, n in ALT_FORMS:
        for layers in (2, 1):
            pre = f"{L}/{layers}/"
            raw = {k[len(pre):]: v for k, v in got.items() if k.startswith(pre)}
            check_stages(_tag(L, layers, dim, heads, suffix), L, layers, dim, heads, ffn, raw, stages=layers == 2)

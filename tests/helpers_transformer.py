"""The transformer expert stage by stage: a plain torch restatement of the architecture in the header of
oracle/esm_oracle.py, written so that every stage can be evaluated from GIVEN inputs (the device's own: teacher forcing),
in fp64 (the reference) or in fp32 with the fp16 rounding points of `EsmOracle(half_points=True)` (`half=True`: used ONLY
as the yardstick -- how far an evaluation that rounds where the device rounds lies from fp64 -- never as the reference).

What pins this file: its fp64 evaluation lies within 1/100 of the fp16 yardstick of an independent ESM-2, the `transformers`
package's port on the same seeded weights (logits, score and input gradient at seven geometries, frozen as
tests/golden/esm_port_*.npz; per layer against the live package: tests/test_esm_port_cpu.py, which also shows the faults that
comparison rejects and the device tests could not). Open: the reference's `esm_one_hot` fork and the real checkpoints' values.

The matrices enter every evaluation at their fp16 values (that quantisation is the specification: the device multiplies
fp16 copies); biases, layer-norm gains and the rotary tables are not quantised. Stages, with the buffer ids of
ppde_debug_transformer_read:

  A   xin_i (0)            -> q|k|v_i (1)                    LN1, the fused q|k|v GEMM, q scaling
  B   xin_i, q|k|v_i       -> xmid_i (3)                     rotary, attention, output projection, residual
  B'  q|k|v of a layer     -> ctx (10)                       the attention alone (the buffer is shared by the layers and the
                                                             backward does not write it: after an evaluation, with or without
                                                             the gradient, it holds the LAST layer's)
  C   xmid_i               -> GELU' (4), xin_{i+1} / xlast (5)   LN2, fc1, GELU, fc2, residual
  D   xlast                -> logits (6)                     final LN, head
  E   logits, tokens       -> score, d logits (7)            tf_score
  F   d embedding (8)      -> d tokens (9)                   the tied embedding GEMM
  G   d tokens, logits     -> gradient on the Potts one-hot  tf_finish_grad: G[token(a)] + log_softmax(logits)[token(a)]

`model()` is the whole network under autograd; it yields what no stage can be fed: d q|k|v of layer 0 (11; the q third is the
gradient w.r.t. the projection BEFORE the q scaling, as the device stores it), d embedding (8) and the gradient.

Rounding points of the half evaluation beyond EsmOracle's, each one the device's own (found by reading tf.h):
  * GELU' is stored in fp16 by the forward GEMM and multiplied into the fp16 gradient by the backward: the
    factor is rounded once more than autograd of the oracle's GELU would (`gelu_grad_fp16`).
  * the energy is the score minus the wild type's, subtracted in fp32 (stage E's `wt_score`).

`mut` (a `Mut`) plants ONE fault of the kind a kernel could have into an evaluation; tests/test_transformer_stages_cpu.py
shows that each lands far outside the bound the GPU tests apply. Four of them (attn_ftz, lse_no_max, lse_plus_max,
online_no_rescale) are invisible on make_esm2_state's magnitudes and seen only on rescaled weights:
tests/test_transformer_range_cpu.py.

The last section restates the persistent GEMMs' tile walk (which output tile a workgroup computes as its first, second, ...)
from the kernels' integer formulas, the GEMM shapes of one evaluation and the row padding: what
tests/test_transformer_population_gpu.py chooses its chains from."""
import collections
import math

import numpy as np
import torch

import esm_oracle as eo

F64, F32 = torch.float64, torch.float32
TAIL = 128            # rows from here on exist only in the 256-residue attention kernels
MARGIN = 4.0          # bound = MARGIN x yardstick (2: the larger of two draws of the same rounding process; 2: margin)

Mut = collections.namedtuple("Mut", "name head chain walk", defaults=(None, None, None))      # walk: a Walk, for faults of the tile walk


def _h(t, half):
    return t.half().to(t.dtype) if half else t


class Params:
    """The state dict as the stages read it. fp16_matrices=False (true fp32 matrices) exists for the identity with
    EsmOracle(half_points=False) only."""

    def __init__(self, state, n_layers, dim, heads, fp16_matrices=True):
        self.p = {k: torch.as_tensor(np.asarray(v), dtype=F32) for k, v in state.items()}
        self.n_layers, self.dim, self.heads, self.hd = n_layers, dim, heads, dim // heads
        self.fp16_matrices = fp16_matrices
        self.perm = torch.as_tensor(eo.potts_to_esm_index())

    def mat(self, name, dtype):
        w = self.p[name]
        return (w.half() if self.fp16_matrices else w).to(dtype)

    def vec(self, name, dtype):
        return self.p[name].to(dtype)


def _pick(mut, mutated, normal):
    """`mutated` on the (chain, head) pairs the mutant is restricted to ([n, H, ...] tensors), `normal` elsewhere."""
    if mut.head is None and mut.chain is None:
        return mutated
    n, H = normal.shape[:2]
    m = torch.ones(n, H, dtype=torch.bool)
    if mut.head is not None:
        m &= (torch.arange(H) == mut.head)[None, :]
    if mut.chain is not None:
        m &= (torch.arange(n) == mut.chain)[:, None]
    return torch.where(m.reshape(n, H, *([1] * (normal.dim() - 2))), mutated, normal)


def _ln(P, x, pre, dtype, mut=None):
    g, b = P.vec(pre + ".weight", dtype), P.vec(pre + ".bias", dtype)
    if mut is not None and mut.name == "ln_bwd_mean_const":      # the backward treats the row mean as a constant
        mu = x.mean(-1, keepdim=True).detach()
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) * torch.rsqrt(var + 1e-5) * g + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def _lin(P, x, pre, dtype, half, bias=True):
    y = _h(x, half) @ P.mat(pre + ".weight", dtype).t()
    if bias:
        y = y + P.vec(pre + ".bias", dtype)
    return _h(y, half)


def _rotary(x, dtype, half, shift_from=None, wrong_grad_sign=False):
    T, hd = x.shape[-2], x.shape[-1]
    inv = 1.0 / (10000 ** (torch.arange(0, hd, 2).to(dtype) / hd))
    pos = torch.arange(T).to(dtype)
    if shift_from is not None:
        pos = pos + (torch.arange(T) >= shift_from).to(dtype)
    fr = torch.outer(pos, inv)
    emb = torch.cat((fr, fr), -1)
    cos, sin = emb.cos(), emb.sin()
    rot = lambda t: torch.cat((-t[..., hd // 2:], t[..., : hd // 2]), -1)
    y = x * cos + rot(x) * sin
    if wrong_grad_sign:                                            # same value; the gradient of the rotation by -angle
        y = (x * cos - rot(x) * sin) + (2.0 * rot(x) * sin).detach()
    return _h(y, half)


class _SoftmaxRowsumCut(torch.autograd.Function):
    """softmax whose backward sums dP o P over the first `keep` keys only (the partial last key tile left out)."""

    @staticmethod
    def forward(ctx, s, keep):
        p = torch.softmax(s, -1)
        ctx.save_for_backward(p)
        ctx.keep = keep
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        return p * (dp - (dp * p)[..., : ctx.keep].sum(-1, keepdim=True)), None


FP16_MIN_NORMAL = 2.0 ** -14


def _ftz(t):
    """fp16 flush-to-zero: magnitudes below the smallest normal become 0 (and pass no gradient)."""
    return torch.where(t.abs() >= FP16_MIN_NORMAL, t, torch.zeros_like(t))


def _softmax_online_no_rescale(s, rise=11.0, tile=16):
    """softmax over key tiles of 16 with a running maximum, whose accumulated weights are NOT rescaled at a tile where the
    maximum rises by more than `rise` (they are at every smaller rise: at such rows it is softmax up to rounding)."""
    m = torch.full_like(s[..., :1], -math.inf)
    total, parts = torch.zeros_like(m), []
    for j in range(0, s.shape[-1], tile):
        sj = s[..., j:j + tile]
        mj = torch.maximum(m, sj.detach().amax(-1, keepdim=True))
        f = torch.where(mj - m > rise, torch.ones_like(m), torch.exp(m - mj))
        parts = [pp * f for pp in parts] + [torch.exp(sj - mj)]
        total, m = total * f + parts[-1].sum(-1, keepdim=True), mj
    return torch.cat(parts, -1) / total


class _GeluStoredGrad(torch.autograd.Function):
    """GELU of an fp16-valued pre-activation, rounded to fp16; the backward multiplies the fp16 gradient by GELU' ROUNDED TO
    fp16, which is what the forward GEMM stores and the backward GEMM's epilogue reads (tf_gelu_both, TF_EPI_GELU_BWD)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(_h(gelu_grad(x), True))
        return _h(gelu(x), True)

    @staticmethod
    def backward(ctx, g):
        gp, = ctx.saved_tensors
        return _h(g, True) * gp


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _act(x, half, gelu_grad_fp16):
    if half and gelu_grad_fp16:
        return _GeluStoredGrad.apply(x)
    return _h(gelu(x), half)


# ---- the stages -----------------------------------------------------------------------------------------------------
def qkv_unscaled(P, i, xin, dtype=F64, half=False, mut=None):
    """LN1 and the three projections, q not yet scaled: [n, L, 3 dim]."""
    pre = f"layers.{i}."
    y = _ln(P, xin.to(dtype), pre + "self_attn_layer_norm", dtype, mut)
    return torch.cat([_lin(P, y, pre + f"self_attn.{nm}_proj", dtype, half) for nm in "qkv"], -1)


def scale_q(P, raw, half=False, mut=None):
    D = P.dim
    ql = raw[..., :D]
    q = ql * (P.hd ** -0.5)
    if mut is not None and mut.name == "dq_no_scale":              # the gradient passes the scaling with factor 1
        q = ql + (q - ql).detach()
    return torch.cat((_h(q, half), raw[..., D:]), -1)


def stage_a(P, i, xin, dtype=F64, half=False, mut=None):
    return scale_q(P, qkv_unscaled(P, i, xin, dtype, half, mut), half, mut)


def attention(P, qkv, dtype=F64, half=False, mut=None):
    """Stage B': q|k|v [n, L, 3 dim] (q scaled) -> ctx [n, L, dim]."""
    qkv = qkv.to(dtype)
    n, L, _ = qkv.shape
    H, hd, D = P.heads, P.hd, P.dim
    name = mut.name if mut is not None else None
    sp = lambda t: t.reshape(n, L, H, hd).transpose(1, 2)
    q, k, v = (sp(qkv[..., j * D:(j + 1) * D]) for j in range(3))
    qr, kr = _rotary(q, dtype, half), _rotary(k, dtype, half)
    if name == "rope_shift_tail":                                  # rows >= 128 rotated by the next row's angle
        qr, kr = _pick(mut, _rotary(q, dtype, half, TAIL), qr), _pick(mut, _rotary(k, dtype, half, TAIL), kr)
    if name == "drot_sign_dk":
        kr = _pick(mut, _rotary(k, dtype, half, wrong_grad_sign=True), kr)
    if name == "attn_ftz":                                         # fp16 subnormals of the MFMA operands read as zero: q, k, v here
        st = lambda t: t + (_ftz(t) - t).detach()                  # (values only: their gradients are products of other operands)
        qr, kr, v = _pick(mut, st(qr), qr), _pick(mut, st(kr), kr), _pick(mut, st(v), v)
    s = qr @ kr.transpose(-1, -2)
    if name == "dk_no_tail":                                       # dK lacks the last query tile's contribution
        s = _pick(mut, torch.cat((s[..., :TAIL, :], qr[..., TAIL:, :] @ kr.detach().transpose(-1, -2)), -2), s)
    s = _h(s, half)
    if name == "tail_no_last_key":                                 # queries of the last tile never see key L - 1
        sm = s.clone()
        sm[..., TAIL:, L - 1] = -math.inf
        s = _pick(mut, sm, s)
    if name == "pad_keys":                                         # keys L .. 16 ceil(L / 16) - 1 admitted with score 0, v 0
        pm = torch.softmax(torch.cat((s, s.new_zeros(n, H, L, -L % 16)), -1), -1)[..., :L]
        p = _pick(mut, pm, torch.softmax(s, -1))
    elif name == "softmax_bwd_rowsum_no_pad_tile":
        p = _pick(mut, _SoftmaxRowsumCut.apply(s, L // 16 * 16), torch.softmax(s, -1))
    elif name == "online_no_rescale":                              # running maximum over key tiles, no rescaling at a rise > 11
        p = _pick(mut, _softmax_online_no_rescale(s), torch.softmax(s, -1))
    else:
        p = torch.softmax(s, -1)
    p = _h(p, half)
    if name == "attn_ftz":                                         # probabilities below 2^-14 are zero in P V and in the backward
        p = _pick(mut, _ftz(p), p)
    ctx = p @ v
    if name == "dv_no_tail":
        ctx = _pick(mut, torch.cat((ctx[..., :TAIL, :], p[..., TAIL:, :] @ v.detach()), -2), ctx)
    return _h(ctx, half).transpose(1, 2).reshape(n, L, D)


def _lin_prev_tile_first_k(P, x, pre, dtype, half, w):
    """_lin as a persistent GEMM would compute it whose first k tile (64 of K) of every later tile of its walk (ordinal >= 1
    in the Walk `w`) still held the A rows of the workgroup's PREVIOUS output tile: rows beyond the chains (pad rows) are zero."""
    n, L, K = x.shape
    W = P.mat(pre + ".weight", dtype)
    a = torch.zeros(w.M_pad, K, dtype=dtype)
    a[: n * L] = _h(x, half).reshape(n * L, K)
    y = a @ W.t()
    for v in np.flatnonzero(w.ordinal >= 1):
        m0, n0 = (int(v) // w.tiles_n) * w.tile_m, (int(v) % w.tiles_n) * w.tile_n
        p0 = (int(w.prev[v]) // w.tiles_n) * w.tile_m
        stale = a[p0:p0 + w.tile_m, :64] - a[m0:m0 + w.tile_m, :64]
        y[m0:m0 + w.tile_m, n0:n0 + w.tile_n] += stale @ W[n0:n0 + w.tile_n, :64].t()
    return _h(y[: n * L].reshape(n, L, -1) + P.vec(pre + ".bias", dtype), half)


def stage_b(P, i, xin, qkv, dtype=F64, half=False, mut=None):
    """-> (ctx_i, xmid_i)."""
    ctx = attention(P, qkv, dtype, half, mut)
    if mut is not None and mut.name == "prev_tile_first_k":
        return ctx, _h(xin.to(dtype) + _lin_prev_tile_first_k(P, ctx, f"layers.{i}.self_attn.out_proj", dtype, half, mut.walk), half)
    return ctx, _h(xin.to(dtype) + _lin(P, ctx, f"layers.{i}.self_attn.out_proj", dtype, half), half)


def stage_c(P, i, xmid, dtype=F64, half=False, mut=None, gelu_grad_fp16=True):
    """-> (GELU' of the fc1 pre-activation [n, L, ffn], the layer's output stream)."""
    pre = f"layers.{i}."
    xmid = xmid.to(dtype)
    hdn = _lin(P, _ln(P, xmid, pre + "final_layer_norm", dtype, mut), pre + "fc1", dtype, half)
    act = _act(hdn, half, gelu_grad_fp16)
    return _h(gelu_grad(hdn.detach()), half), _h(xmid + _lin(P, act, pre + "fc2", dtype, half), half)


def stage_d(P, xlast, dtype=F64, half=False, mut=None, gelu_grad_fp16=True):
    x = _ln(P, xlast.to(dtype), "emb_layer_norm_after", dtype, mut)
    y = _act(_lin(P, x, "lm_head.dense", dtype, half), half, gelu_grad_fp16)
    y = _ln(P, y, "lm_head.layer_norm", dtype, mut)
    return _h(_h(y, half) @ P.mat("embed_tokens.weight", dtype).t() + P.vec("lm_head.bias", dtype), half)


def stage_e(P, logits, idx, dtype=F64, half=False, wt_score=None, mut=None):
    """logits [n, L, 33], idx [n, L] Potts letters -> (score [n], d score / d logits [n, L, 33]). With wt_score (the
    device's own wild-type score, an input like the tokens) the first is the energy score - wt_score, which the half
    evaluation subtracts in fp32 as the device does. The score is ONE number per chain, and in fp32 its distance from fp64
    is the rounding of the sum over the residues alone: the half evaluation adds them one after the other, the plainest
    order and one that does not depend on the host's reduction kernels (the device's fixed tree is another order of the
    same sum)."""
    lp = torch.log_softmax(logits.to(dtype), -1)
    if mut is not None and mut.name == "lse_no_max":               # log-sum-exp without the row maximum subtracted
        lg = logits.to(dtype)
        lp = lg - lg.exp().sum(-1, keepdim=True).log()
    if mut is not None and mut.name == "lse_plus_max":             # v - (log s + max): the sum rounded at the logits' magnitude
        lg = logits.to(dtype)                                      # (what tf_score did until the range tests ran it at logits of 60)
        mx = lg.amax(-1, keepdim=True)
        lp = lg - ((lg - mx).exp().sum(-1, keepdim=True).log() + mx)
    onehot = torch.nn.functional.one_hot(P.perm[torch.as_tensor(np.asarray(idx)).long()], 33).to(dtype)
    rows = (onehot * lp).sum(-1)                                   # [n, L]: one non-zero term each
    if half:
        s = torch.zeros_like(rows[:, 0])
        for l in range(rows.shape[1]):
            s = s + rows[:, l]
    else:
        s = rows.sum(1)
    if wt_score is not None:
        s = s - torch.tensor(float(wt_score), dtype=F64).to(dtype)
    return s, _h(onehot - lp.exp(), half)


def stage_f(P, demb, dtype=F64, half=False):
    """d score / d (one-hot @ E) [n, L, dim] -> d score / d tokens [n, L, 33] through the embedding."""
    return _h(_h(demb.to(dtype), half) @ P.mat("embed_tokens.weight", dtype).t(), half)


def stage_g(P, dtok, logits, dtype=F64, half=False):
    """-> the gradient on the Potts one-hot [n, L, 20]: the path through the network plus the explicit x in
    sum x * log_softmax (tf_score's gdirect, computed from the fp16 logits in fp32 and never rounded)."""
    return dtok.to(dtype)[..., P.perm] + torch.log_softmax(logits.to(dtype), -1)[..., P.perm]


def model(P, idx, dtype=F64, half=False, mut=None, gelu_grad_fp16=True, want_grad=True):
    """The whole network on Potts letters idx [n, L]. Returns a dict: score, every stage's output (xin{i}, qkv{i}, ctx{i},
    xmid{i}, gp{i}, xlast, logits) and, with want_grad, grad [n, L, 20], demb and dqkv0."""
    idx = torch.as_tensor(np.asarray(idx)).long()
    x_potts = torch.nn.functional.one_hot(idx, 20).to(dtype).requires_grad_(want_grad)
    Pm = torch.zeros(20, 33, dtype=dtype)
    Pm[torch.arange(20), P.perm] = 1.0
    x_esm = x_potts @ Pm
    emb = _h(x_esm, half) @ P.mat("embed_tokens.weight", dtype)
    x = _h(_h(emb, half) * eo.TOKEN_DROPOUT_SCALE, half)
    out, raw0 = {}, None
    for i in range(P.n_layers):
        out[f"xin{i}"] = x
        raw = qkv_unscaled(P, i, x, dtype, half, mut)
        if i == 0:
            raw0 = raw
            if want_grad:
                raw0.retain_grad()
        qkv = scale_q(P, raw, half, mut)
        ctx, x = stage_b(P, i, x, qkv, dtype, half, mut)
        out[f"qkv{i}"], out[f"ctx{i}"], out[f"xmid{i}"] = qkv, ctx, x
        out[f"gp{i}"], x = stage_c(P, i, x, dtype, half, mut, gelu_grad_fp16)
    out["xlast"] = x
    lg = out["logits"] = stage_d(P, x, dtype, half, mut, gelu_grad_fp16)
    s = (x_esm * torch.log_softmax(lg, -1)).sum(dim=[1, 2])
    if want_grad:
        emb.retain_grad()
        s.sum().backward()
        out["grad"], out["demb"], out["dqkv0"] = x_potts.grad, emb.grad, raw0.grad
    out["score"] = s
    return {k: v.detach() for k, v in out.items()}


# ---- measures (no row, head, chain or stage is exempted) -------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.asarray(a)).to(F64)


def row_rel(got, ref):
    """Activations and teacher-forced outputs [n, L, d]: the largest ||got_row - ref_row|| / ||ref_row||."""
    got, ref = _t(got), _t(ref)
    return float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max())


def slice_rel(got, ref, hd, thirds=1):
    """ctx [n, L, dim] (thirds=1) and d q|k|v [n, L, 3 dim] (thirds=3): the error of every (row, head slice), per third of
    q|k|v, over that third's largest row norm in the chain."""
    got, ref = _t(got), _t(ref)
    n, L, W = ref.shape
    D = W // thirds
    worst = 0.0
    for j in range(thirds):
        g, r = got[..., j * D:(j + 1) * D], ref[..., j * D:(j + 1) * D]
        err = (g - r).reshape(n, L, D // hd, hd).norm(dim=-1)                       # [n, L, H]
        worst = max(worst, float((err / r.norm(dim=-1).amax(dim=1)[:, None, None]).max()))
    return worst


def chain_rel(got, ref):
    """Gradient and d embedding [n, L, d]: per chain, the largest row error over that chain's largest row norm."""
    got, ref = _t(got), _t(ref)
    return float(((got - ref).norm(dim=-1).amax(dim=1) / ref.norm(dim=-1).amax(dim=1)).max())


def score_rel(got, ref, scale=None):
    """|delta| / |s| (scale: the raw scores, where got / ref are energies against the wild type)."""
    got, ref = _t(got), _t(ref)
    return float(((got - ref).abs() / (_t(scale) if scale is not None else ref).abs()).max())


# ---- the independent pin: tests/golden/esm_port_<tag>.npz hold what the `transformers` package's ESM-2 port computes (fp64, matrices
# at their fp16 values) on make_esm2_state(seed=ESM_PORT_WEIGHT_SEED) and chains_like_the_parity_test(L, n); see tests/helpers_esm_port.py
#                     (L, layers, dim, heads, ffn, chains)
ESM_PORT_GEOMETRIES = [(17, 2, 128, 4, 256, 3),          # short sequence
                       (129, 2, 128, 4, 256, 3),         # one row past 128
                       (237, 2, 96, 4, 256, 2),          # head width 24, pad keys
                       (129, 2, 256, 4, 512, 2),         # head width 64
                       (104, 2, 480, 20, 1920, 2),       # 35M widths
                       (256, 2, 128, 2, 256, 2),         # the longest sequence, rotary to position 255
                       (104, 30, 640, 20, 2560, 2)]      # the 150M model at its full depth
ESM_PORT_WEIGHT_SEED = 3


def esm_port_tag(L, layers, dim, heads, ffn=None, n=None):
    return f"{L}x{layers}x{dim}x{heads}"


def chains_like_the_parity_test(L, n, seed=3):
    """The wild type and n chains perturbed as in test_score_and_gradient_vs_oracle: chain b differs at 3 b residues."""
    wt = np.random.default_rng(seed).integers(0, 20, L).astype(np.uint8)
    rng = np.random.default_rng(L)
    idx = np.tile(wt, (n, 1))
    for b in range(1, n):
        pos = rng.choice(L, size=min(L, 3 * b), replace=False)
        idx[b, pos] = rng.integers(0, 20, len(pos))
    return wt, idx


# ---- the persistent GEMMs' tile walk, restated on the CPU (tf.h: tf_gemm_nt, tf_gemm160, tf_gemm_big; tf_host.h: tf_gemm) -------
# Per output tile v (N-fastest order): its ordinal in its workgroup's walk (ti // wpx), the XCD whose run it lies in, the
# workgroup, the tile that workgroup computed before it (-1: none) and how many workgroups visit it.
Walk = collections.namedtuple("Walk", "ordinal xcd block prev visits grid M_pad tiles_n tile_m tile_n")

#              L   dim heads ffn  chains: the smallest shapes at which every GEMM with N >= 256 gives a workgroup a second tile
POPULATIONS = {"P160": (104, 640, 20, 1280, 256),      # tf_gemm160 (every width a multiple of 160)
               "P128": (237, 256, 8, 512, 198)}        # tf_gemm_nt (128-row tiles); 198 chains, not 192: with 192 the 14 tiles at
#                                                        ordinal 4 of N = 768 (2.3 row tiles) hold no chain of 237 rows entirely


def pad_rows(M, use160=True, big=False):
    """tf_pad_rows: the token rows padded to whole row tiles of every GEMM kernel in use."""
    g = (1280 if big else 640) if use160 else (256 if big else 128)
    return (M + g - 1) // g * g


def walk(M_pad, N, tile, cap=512):
    """The kernels' integer formulas, workgroup by workgroup. tile: the edge of a square tile, or (rows, columns)."""
    tile_m, tile_n = (tile, tile) if isinstance(tile, int) else tile
    assert M_pad % tile_m == 0 and N % tile_n == 0
    tiles_n = N // tile_n
    tiles_total = (M_pad // tile_m) * tiles_n
    tiles8 = (tiles_total + 7) & ~7
    grid = min(tiles8, cap)                                          # (tf_host.h: the launch)
    ordinal, xcd_of, block_of, prev = (np.full(tiles_total, -1, np.int64) for _ in range(4))
    visits = np.zeros(tiles_total, np.int64)
    wpx = grid >> 3
    xq, xr = tiles_total >> 3, tiles_total & 7
    for block in range(grid):
        xcd, slot = block & 7, block >> 3
        xbeg, xcnt = xcd * xq + min(xcd, xr), xq + (1 if xcd < xr else 0)
        for ti in range(slot, xcnt, wpx):
            v = xbeg + ti
            visits[v] += 1
            ordinal[v], xcd_of[v], block_of[v] = ti // wpx, xcd, block
            prev[v] = v - wpx if ti - wpx >= slot else -1
    return Walk(ordinal, xcd_of, block_of, prev, visits, grid, M_pad, tiles_n, tile_m, tile_n)


def tile_walk(M_pad, N, tile, cap=512):
    """For every output tile v (row tile m0 = v // tiles_n): its ordinal in its workgroup's walk."""
    return walk(M_pad, N, tile, cap).ordinal


def gemm_shapes(dim, ffn, M_pad, use160=True):
    """Every GEMM an evaluation with the gradient launches (tf_eval_chunk), forward then backward, as
    (name, N, K, tile, kernel): tf_gemm160 where M and N are multiples of 160 (and PPDE_TF_160 is not 0), else tf_gemm_nt."""
    D, V = (dim + 127) // 128 * 128, 128
    launches = [("qkv", 3 * D, D), ("out_proj", D, D), ("fc1", ffn, D), ("fc2", D, ffn), ("head_dense", D, D), ("logits", V, D),
                ("logits.bwd", D, V), ("head_dense.bwd", D, D), ("fc2.bwd", ffn, D), ("fc1.bwd", D, ffn), ("out_proj.bwd", D, D),
                ("qkv.bwd", D, 3 * D), ("embedding.bwd", V, D)]
    out = []
    for name, N, K in launches:
        t160 = use160 and M_pad % 160 == 0 and N % 160 == 0
        out.append((name, N, K, 160 if t160 else 128, "tf_gemm160" if t160 else "tf_gemm_nt"))
    return out


def _chain_row_tiles(w, L, c):
    return range(c * L // w.tile_m, ((c + 1) * L - 1) // w.tile_m + 1)


def select_chains(L, n, dim, ffn):
    """The chains whose stages the population tests bound against fp64, chosen from the walk of the geometry's GEMM shapes:
    chain 0, the last chain, for every shape (N, tile) and every ordinal >= 1 it reaches one chain whose rows lie wholly in
    tiles of that ordinal, one chain holding the first row of a workgroup's second tile and one whose rows straddle two
    XCDs' runs (both in the N = dim GEMM). -> (sorted chains, {chain: [reasons]}, [(N, tile, ordinal) without a chain])."""
    M_pad = pad_rows(n * L)
    D = (dim + 127) // 128 * 128
    shapes = sorted({(N, tile) for _, N, _, tile, _ in gemm_shapes(dim, ffn, M_pad)}, key=lambda s: (s[0] != D, s[0]))
    why, missing = {0: ["the wild type"]}, []
    why.setdefault(n - 1, []).append("the last chain, beside the pad rows")
    grids = {}
    for N, tile in shapes:
        w = walk(M_pad, N, tile)
        o = w.ordinal.reshape(-1, w.tiles_n)
        lo = np.array([min(o[r].min() for r in _chain_row_tiles(w, L, c)) for c in range(n)])
        hi = np.array([max(o[r].max() for r in _chain_row_tiles(w, L, c)) for c in range(n)])
        grids[(N, tile)] = (w, lo, hi)
        for k in range(1, int(w.ordinal.max()) + 1):
            fit = [c for c in range(n) if lo[c] == hi[c] == k]
            if not fit:
                missing.append((N, tile, k))
                continue
            c = next((c for c in fit if c not in why), fit[0])          # a chain of its own where there is one
            why.setdefault(c, []).append(f"wholly in ordinal {k} of N = {N}, {tile}-tiles")
    w, lo, hi = grids[shapes[0]]                                     # the N = dim GEMM
    x = w.xcd.reshape(-1, w.tiles_n)
    first2 = np.flatnonzero(w.ordinal == 1)
    if len(first2):
        c = (int(first2[0]) // w.tiles_n) * w.tile_m // L            # the chain that holds that tile's first row
        if c < n:
            why.setdefault(c, []).append(f"holds the first row of a workgroup's second tile (N = {shapes[0][0]})")
    for c in range(n):
        if len({int(t) for r in _chain_row_tiles(w, L, c) for t in x[r]}) > 1:
            why.setdefault(c, []).append(f"straddles two XCDs' runs (N = {shapes[0][0]})")
            break
    return sorted(why), why, missing

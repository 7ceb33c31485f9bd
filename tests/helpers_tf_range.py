"""The transformer expert across the dynamic range of its weights: rescalings of a `synthetic.make_esm2_state` dict (pure
functions, the input is never modified), the geometries and cases the range tests run, and the ranges themselves.

Function-preserving families (the fp64 function is unchanged up to the layer norms' epsilon; s = 2^exponent):
  stream   the whole residual stream x s: embedding, every out_proj and fc2 (weight and bias) x s, the head's layer norm
           (weight and bias) / s -- the embedding is also the tied head projection, so the logits stay where they were
  qk       q_proj x s, k_proj / s (weights and biases)
  vo       v_proj x s (weight and bias), out_proj weight / s
  lngain   self_attn_layer_norm x s with the q, k, v weights / s; final_layer_norm x s with the fc1 weight / s
Peaked families (another function; fp64 on the same weights is still the reference):
  sharp    q_proj and k_proj both x s: the scores x s^2
  head     the head's layer-norm gain x s: the logits x s
  channel  one stream channel x s: that column of the embedding, that row of every out_proj and fc2 weight, that bias entry

RANGE, PEAKED and the unit-scale figures are asserted by tests/test_transformer_range_cpu.py, which recomputes them from
tests/helpers_transformer.py alone (fp64 against the evaluation that rounds where the device rounds), never from device
output; tests/test_transformer_range_gpu.py runs the device at the cases listed here."""
import functools

import numpy as np

import helpers_transformer as ht
from helpers_transformer import F32, F64
from ppde_amd import synthetic

PRESERVING = ("stream", "qk", "vo", "lngain")
PEAKED_FAMILIES = ("sharp", "head", "channel")
CHANNEL = 5                       # the stream channel that `channel` scales
SEED = 3                          # make_esm2_state's seed in every transformer test


def _scaled(st, names, s):
    for k in names:
        st[k] = (np.asarray(st[k], np.float32) * np.float32(s)).astype(np.float32)


def regime(state, family, exponent, layers):
    """A copy of `state` rescaled by s = 2^exponent in the way of `family` (exact: powers of two)."""
    st = {k: np.array(v, np.float32, copy=True) for k, v in state.items()}
    s, r = 2.0 ** exponent, 2.0 ** -exponent
    lay = [f"layers.{i}." for i in range(layers)]
    wb = lambda pre: [pre + ".weight", pre + ".bias"]
    if family == "stream":
        _scaled(st, ["embed_tokens.weight"], s)
        for p in lay:
            _scaled(st, wb(p + "self_attn.out_proj") + wb(p + "fc2"), s)
        _scaled(st, wb("lm_head.layer_norm"), r)
    elif family == "qk":
        for p in lay:
            _scaled(st, wb(p + "self_attn.q_proj"), s)
            _scaled(st, wb(p + "self_attn.k_proj"), r)
    elif family == "vo":
        for p in lay:
            _scaled(st, wb(p + "self_attn.v_proj"), s)
            _scaled(st, [p + "self_attn.out_proj.weight"], r)
    elif family == "lngain":
        for p in lay:
            _scaled(st, wb(p + "self_attn_layer_norm") + wb(p + "final_layer_norm"), s)
            _scaled(st, [p + f"self_attn.{nm}_proj.weight" for nm in "qkv"] + [p + "fc1.weight"], r)
    elif family == "sharp":
        for p in lay:
            _scaled(st, wb(p + "self_attn.q_proj") + wb(p + "self_attn.k_proj"), s)
    elif family == "head":
        _scaled(st, ["lm_head.layer_norm.weight"], s)
    elif family == "channel":
        c = CHANNEL
        st["embed_tokens.weight"][:, c] *= np.float32(s)
        for p in lay:
            for nm in ("self_attn.out_proj", "fc2"):
                st[p + nm + ".weight"][c, :] *= np.float32(s)
                st[p + nm + ".bias"][c] *= np.float32(s)
    else:
        raise ValueError(family)
    return st


def letter_overflow(state, letter):
    """A copy of `state` on which a chain goes non-finite if and only if it holds Potts letter `letter`. Behind a pre-layer-norm
    block nothing but the residual stream itself can leave fp16's range, and an embedding entry cannot do it alone (it is at most
    65504, and enters the stream x 0.88). So: the largest entry of the letter's embedding row, channel c, becomes +-65504 (the
    stream holds +-57644 there); layer 0's out_proj bias adds +-8192 in channel c, which every other row carries with ease and
    this one does not (65836 rounds to inf); and the head's layer norm passes nothing of channel c (gain and bias 0), because the
    embedding is also the head's projection: its entry of 65504 would otherwise overflow that letter's logit in EVERY chain."""
    import esm_oracle as eo
    st = {k: np.array(v, np.float32, copy=True) for k, v in state.items()}
    row = int(eo.potts_to_esm_index()[letter])
    c = int(np.abs(st["embed_tokens.weight"][row]).argmax())
    sign = np.float32(np.sign(st["embed_tokens.weight"][row, c]))
    st["embed_tokens.weight"][row, c] = sign * np.float32(65504.0)
    st["layers.0.self_attn.out_proj.bias"][c] = sign * np.float32(8192.0)
    st["lm_head.layer_norm.weight"][c] = st["lm_head.layer_norm.bias"][c] = 0.0
    return st


# ---- geometries (L, dim, heads, ffn, chains) and the cases of each ------------------------------------------------------------
GEOMS = {"17x128": (17, 128, 4, 256, 3),          # head width 32, 128-residue attention
         "129x256": (129, 256, 4, 512, 2),        # head width 64, 256-residue attention, two key halves
         "24x96": (24, 96, 4, 256, 3),            # head width 24
         "237x96": (237, 96, 4, 256, 2),          # pad keys in the last tile under peaked rows
         "24x768": (24, 768, 12, 1024, 3),        # the other layer-norm kernels
         "24x1536": (24, 1536, 24, 1024, 3)}      # the widest layer-norm row
FAMILIES_OF = {"17x128": PRESERVING + PEAKED_FAMILIES,
               "129x256": PRESERVING + PEAKED_FAMILIES,
               "24x96": ("qk", "vo", "sharp"),
               "237x96": ("sharp",),
               "24x768": ("stream", "lngain", "channel"),
               "24x1536": ("stream", "lngain", "channel")}
RANGE_GEOMS = ("17x128", "129x256", "24x96", "24x768")      # the geometries the supported ranges are computed on
YARDSTICKS = ("model.grad", "model.demb", "model.dqkv0", "model.score")
SEARCH = 18                       # the search walks outwards from exponent 0 to +- this

# The supported range of each function-preserving family: the exponents, contiguous from 0, at which on every geometry of
# RANGE_GEOMS that runs the family (two layers) the half-points evaluation is finite and model.grad, model.demb and model.dqkv0
# each lie within 2 x their unit-scale value on the same geometry and chains, and model.score does over the geometries together
# (admitted(), below). At 24x1536 the edges are checked to be admitted too.
RANGE = {"stream": (-12, 12), "qk": (-12, 13), "vo": (-14, 13), "lngain": (-14, 11)}
# The first exponent past the high edge at which the half-points evaluation is no longer finite on ANY geometry of the family
# (an fp16 activation beyond 65504): what the device is run at "past the edge".
OVERFLOW = {"stream": 14, "lngain": 14}
# The peaked exponents that go to the device: the largest at which the bounds still reject every live mutant of the stage tables
# (verdict(), below).
PEAKED = {"sharp": 2, "head": 4, "channel": 3}
# What makes a peaked case peaked, under fp64: sharp -- every head has a row with a probability above 0.9 and, in such a row, one
# below fp16's smallest normal; head -- a logit beyond 50 in magnitude; channel -- the scaled channel carries more than half of some
# stream row's energy at widths 128 and 256. A share of 0.9 is out of reach: the exponent that keeps the bounds' teeth (3) gives
# 0.72 / 0.69 there, and 0.30 / 0.23 of a row of 768 / 1536 channels.
PEAKED_SHARE = {"17x128": 0.5, "129x256": 0.5, "24x768": 0.2, "24x1536": 0.2}


def range_geoms(family):
    return [g for g in RANGE_GEOMS if family in FAMILIES_OF[g]]


def state(geom, layers):
    L, dim, heads, ffn, n = GEOMS[geom]
    return synthetic.make_esm2_state(layers, dim, heads, ffn, seed=SEED)


def exponents(geom, family):
    """The exponents of `family` that the device runs at on `geom`: both edges of a supported range, or the peaked exponent."""
    return RANGE[family] if family in RANGE else (PEAKED[family],)


CASES = [(g, f, e) for g in GEOMS for f in FAMILIES_OF[g] for e in exponents(g, f)]


def _finite(out):
    return all(bool(np.isfinite(np.asarray(v)).all()) for v in out.values())


def evaluate(geom, layers, family=None, exponent=0, half_dtype=F64):
    """(Params, idx, fp64 model, half-points model) of one case; family None: unit scale. The half-points evaluation rounds to
    fp16 where the device does and is otherwise carried in `half_dtype`. F64 (what RANGE and PEAKED are computed with): sums of
    products of fp16 values are then exact or as good as exact, so the result does not depend on the host's BLAS, its threads or
    its reduction order, and the committed edges are the same on every machine. F32 is what check_stages uses as its yardstick:
    another draw of the same rounding process, whose fp32 sums do depend on the host."""
    L, dim, heads, ffn, n = GEOMS[geom]
    st = state(geom, layers)
    if family is not None:
        st = regime(st, family, exponent, layers)
    P = ht.Params(st, layers, dim, heads)
    _, idx = ht.chains_like_the_parity_test(L, n)
    return P, idx, ht.model(P, idx, F64), ht.model(P, idx, half_dtype, half=True)


ROW_YARDSTICKS = ("model.grad", "model.demb", "model.dqkv0")       # maxima over every row of every chain


def yardsticks(P, ref, half):
    """The whole-model yardsticks of check_stages, with every chain's score distance, or None where an evaluation is not finite."""
    if not _finite(half) or not _finite(ref):
        return None
    return {"model.grad": ht.chain_rel(half["grad"], ref["grad"]), "model.demb": ht.chain_rel(half["demb"], ref["demb"]),
            "model.dqkv0": ht.slice_rel(half["dqkv0"], ref["dqkv0"], P.hd, 3), "model.score": ht.score_rel(half["score"], ref["score"]),
            "scores": ((half["score"] - ref["score"]).abs() / ref["score"].abs()).numpy()}


@functools.lru_cache(maxsize=None)
def case_yardsticks(geom, layers, family=None, exponent=0, half_dtype=F64):
    P, _, ref, half = evaluate(geom, layers, family, exponent, half_dtype)
    return yardsticks(P, ref, half)


def rows_admitted(geom, family, exponent, layers=2):
    """Finite, and each yardstick that is a maximum over rows within 2 x its unit-scale value on the same geometry and chains."""
    y, unit = case_yardsticks(geom, layers, family, exponent), case_yardsticks(geom, layers)
    return y is not None and all(np.isfinite(y[k]) and y[k] <= 2.0 * unit[k] for k in ROW_YARDSTICKS)


def pooled_score(geoms, family=None, exponent=0, layers=2):
    """model.score is ONE number per chain: on two or three chains its largest value is a draw that varies by more than the factor
    2 from one regime to the next with nothing changed (and is 0.3 to 3 times its unit-scale value all over every range, on one
    geometry or another). What the criterion holds to 2 x its unit-scale value is the root mean square of the chains' score
    distances over the family's geometries: eight or more draws."""
    ys = [case_yardsticks(g, layers, family, exponent) for g in geoms]
    if any(y is None for y in ys):
        return np.inf
    return float(np.sqrt(np.mean(np.concatenate([y["scores"] for y in ys]) ** 2)))


def admitted(family, exponent):
    """The supported-range criterion of a function-preserving family at one exponent."""
    geoms = range_geoms(family)
    return all(rows_admitted(g, family, exponent) for g in geoms) and pooled_score(geoms, family, exponent) <= 2.0 * pooled_score(geoms)


def family_geoms(family):
    return [g for g in GEOMS if family in FAMILIES_OF[g]]


# ---- what the bounds reject inside the range: the mutants of tests/test_transformer_stages_cpu.py on rescaled weights ----------
MUTANT_GEOM = (128, 4, 256, 3)    # dim, heads, ffn, chains of that module's _setup
HALF = F64                        # what carries the half-points evaluations here between their fp16 rounding points (see evaluate())


@functools.lru_cache(maxsize=None)
def mutant_setup(L, layers, family=None, exponent=0, geom=MUTANT_GEOM):
    """test_transformer_stages_cpu._setup on rescaled weights: (Params, idx, fp64 model, half-points model)."""
    dim, heads, ffn, n = geom
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=SEED)
    if family is not None:
        st = regime(st, family, exponent, layers)
    P = ht.Params(st, layers, dim, heads)
    _, idx = ht.chains_like_the_parity_test(L, n)
    return P, idx, ht.model(P, idx, F64), ht.model(P, idx, HALF, half=True)


def _far(d):
    return d if np.isfinite(d) else np.inf                          # a non-finite evaluation is infinitely far


def stage_b_distances(L, mut, family=None, exponent=0, geom=MUTANT_GEOM):
    """Per layer of a two-layer model, in stage B's measure and on the half-points model's own inputs: (the yardstick, the
    half-points mutant's distance from fp64, the distance of the mutant planted into fp64 itself)."""
    P, idx, _, hm = mutant_setup(L, 2, family, exponent, geom)
    res = []
    for i in range(2):
        xin, qkv = hm[f"xin{i}"], hm[f"qkv{i}"]
        ref = ht.stage_b(P, i, xin, qkv, F64)[1]
        res.append((ht.row_rel(ht.stage_b(P, i, xin, qkv, HALF, True)[1], ref),
                    _far(ht.row_rel(ht.stage_b(P, i, xin, qkv, HALF, True, mut)[1], ref)),
                    _far(ht.row_rel(ht.stage_b(P, i, xin, qkv, F64, False, mut)[1], ref))))
    return res


def backward_distances(L, mut, family=None, exponent=0, geom=MUTANT_GEOM):
    """One layer, the whole model under autograd: the same triple for (gradient, d q|k|v of layer 0)."""
    P, idx, ref, hm = mutant_setup(L, 1, family, exponent, geom)
    mm, m64 = ht.model(P, idx, HALF, half=True, mut=mut), ht.model(P, idx, F64, mut=mut)
    dq = lambda a: ht.slice_rel(a["dqkv0"], ref["dqkv0"], P.hd, 3)
    return [(ht.chain_rel(hm["grad"], ref["grad"]), _far(ht.chain_rel(mm["grad"], ref["grad"])), _far(ht.chain_rel(m64["grad"], ref["grad"]))),
            (dq(hm), _far(dq(mm)), _far(dq(m64)))]


def stage_e_distances(L, mut, family=None, exponent=0, geom=MUTANT_GEOM):
    """Stage E on the half-points model's logits: the same triple for (score, d logits). Stage E is fp32 arithmetic on fp16 logits on
    the device, and its yardstick is that of fp32 (carried in fp64 it would be zero for the score)."""
    P, idx, _, hm = mutant_setup(L, 2, family, exponent, geom)
    lg = hm["logits"]
    r, h = ht.stage_e(P, lg, idx, F64), ht.stage_e(P, lg, idx, F32, True)
    m, m64 = ht.stage_e(P, lg, idx, F32, True, mut=mut), ht.stage_e(P, lg, idx, F64, mut=mut)
    return [(ht.score_rel(h[0], r[0]), _far(ht.score_rel(m[0], r[0])), _far(ht.score_rel(m64[0], r[0]))),
            (ht.row_rel(h[1], r[1]), _far(ht.row_rel(m[1], r[1])), _far(ht.row_rel(m64[1], r[1])))]


def verdict(distances, unit_distances):
    """(rejected, live, multiples) of one mutant at one regime, from its distances there and at unit scale.
    rejected: one of the bounds that catch it at unit scale rejects it (distance > MARGIN x this regime's yardstick);
    live: the fault is still in the function -- planted into fp64 it moves the result by more than MARGIN x the UNIT-scale
    yardstick of a bound that catches it (a bound as tight as at unit scale would see it). A fault that the regime itself removes
    (the last key's weight under peaked rows, any key's under identical keys) is not live, and no bound can be asked to see it."""
    mult = [d / y for y, d, _ in distances]
    rejected = any(m > ht.MARGIN for m in mult)
    live = any(f > ht.MARGIN * u[0] for (_, _, f), u in zip(distances, unit_distances))
    return rejected, live, mult


# ---- is a peaked case peaked (fp64) ----------------------------------------------------------------------------------------
def attention_probs(P, qkv):
    """The fp64 attention probabilities [n, H, L, L] of a layer's q|k|v (q scaled), as helpers_transformer.attention forms them."""
    import torch
    qkv = qkv.to(F64)
    n, L, _ = qkv.shape
    sp = lambda t: t.reshape(n, L, P.heads, P.hd).transpose(1, 2)
    q, k = (sp(qkv[..., j * P.dim:(j + 1) * P.dim]) for j in range(2))
    return torch.softmax(ht._rotary(q, F64, False) @ ht._rotary(k, F64, False).transpose(-1, -2), -1)


def peakedness(geom, family, exponent, layers=2):
    """sharp: per head (over layers, chains), the largest row maximum and the smallest entry of a row whose maximum is above
    0.9; head: the largest |logit|; channel: the largest share of a stream row's energy that channel CHANNEL carries."""
    P, idx, ref, _ = evaluate(geom, layers, family, exponent)
    if family == "sharp":
        top, low = np.zeros(P.heads), np.ones(P.heads)
        for i in range(layers):
            p = attention_probs(P, ref[f"qkv{i}"])
            rmax, rmin = p.amax(-1), p.amin(-1)                                  # [n, H, L]
            for h in range(P.heads):
                top[h] = max(top[h], float(rmax[:, h].max()))
                sel = rmax[:, h] > 0.9
                if sel.any():
                    low[h] = min(low[h], float(rmin[:, h][sel].min()))
        return top, low
    if family == "head":
        return float(ref["logits"].abs().max())
    rows = [ref[k] for k in ref if k.startswith(("xin", "xmid", "xlast"))]
    return max(float((x[..., CHANNEL] ** 2 / (x ** 2).sum(-1)).max()) for x in rows)

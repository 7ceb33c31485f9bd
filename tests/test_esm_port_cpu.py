"""The ESM-2 arithmetic pinned to an independent implementation: the `transformers` package's port (tests/helpers_esm_port.py)
on this project's seeded weights, frozen as tests/golden/esm_port_<geometry>.npz (logits, score, gradient on the Potts one-hot;
fp64, matrices at their fp16 values; made by `tests/golden/make_golden.py esm_port`).

  a. golden (always run, every fixture): the fp64 reference of every device bound, helpers_transformer.model(P, idx, F64), lies
     within 1/100 of the fp16 yardstick of the fixture; EsmOracle(half_points=True) within 4 x that yardstick. The yardstick
     of a quantity is the distance, in the same measure, of model(P, idx, F32, half=True) from the FIXTURE. Why 1/100: every
     device bound of the suite is 4 x a yardstick, so a reference under 1 % of a yardstick from the independent one is
     interchangeable with it for all of them. Measured: 3e-5 .. 8e-4 of a yardstick (the port rotates q and k in fp32
     whatever its dtype; nothing else separates the two).
  b. live (skipped without the package): the name map is total, the ids path equals the embeds path bit for bit, a fresh
     evaluation reproduces the fixtures to 1e-9, every layer's input / the final layer norm / the attention probabilities
     match the port's per layer, the fp32 oracle matches the fp64 port as well as the fp32 port does, and the size of the
     half-points oracle's rounding is that of the port under autocast.
  c. what the comparison rejects (fixtures only): one fault at a time planted into the fp64 helper by monkeypatching; each
     must lie at >= 10 x the 1/100-yardstick bound in some measure at every two-layer geometry. Measured distances from the
     fixture (lowest .. highest over the six geometries, each time the measure that shows the fault best), as multiples of
     the 1/100-yardstick bound | of the 4 x yardstick device bound:

         tanh-GELU in place of erf-GELU                   37 .. 215        |  0.09 .. 0.54
         no token-dropout scale                         3500 .. 4130       |  8.7 .. 10.3
         rotary: keys' positions from 1                10300 .. 28300      |   26 .. 71
         interleaved-pair rotary                       54300 .. 179000     |  136 .. 448
         dim^-0.5 query scaling                        41500 .. 294000     |  104 .. 734
         layer-norm eps 1e-12                            138 .. 561        |  0.35 .. 1.4
         lm_head.bias missing                            790 .. 1290       |  2.0 .. 3.2
         post-LN residual order                        84400 .. 161000     |  211 .. 404

     Under 1 in the second column means: had all three of this project's statements of ESM-2 shared the fault, the device
     tests alone (device against the project's own fp64 within 4 x yardstick) could not have seen it. That holds for
     tanh-GELU at every geometry, and for layer-norm eps 1e-12 at five of the six (the score of 129x2x128x4 reaches 1.4).
     "Rotary positions from 1" needs a word. Rotating queries AND keys from position 1 changes nothing: rotary attention
     sees only position differences, and the helper so changed equals itself to 1e-12
     (test_a_common_rotary_offset_is_invisible states that as a fact, so that nobody reads the table as covering it). What
     an off-by-one in a rotary table can make wrong is the offset BETWEEN queries and keys; that is the fault planted."""
import functools
import math

import numpy as np
import pytest
import torch

import esm_oracle as eo
import helpers_transformer as ht
from helpers import load
from helpers_transformer import F32, F64
from ppde_amd import synthetic

GEOMS = ht.ESM_PORT_GEOMETRIES
TWO_LAYER = [g for g in GEOMS if g[1] == 2]
IDS = [ht.esm_port_tag(*g) for g in GEOMS]
IDS2 = [ht.esm_port_tag(*g) for g in TWO_LAYER]
MEASURES = (("logits", ht.row_rel), ("score", ht.score_rel), ("grad", ht.chain_rel))
PIN = 1.0 / 100           # the reference's bound, in yardsticks
FAULT_CLEARS = 10.0       # a planted fault must exceed that bound this many times in some measure


@functools.lru_cache(maxsize=None)
def _case(geom):
    """The fixture, the inputs it was made from, the fp64 helper's evaluation and the yardsticks (against the FIXTURE)."""
    L, layers, dim, heads, ffn, n = geom
    fx = load(f"esm_port_{ht.esm_port_tag(*geom)}.npz")
    assert tuple(int(v) for v in fx["geometry"]) == geom and int(fx["weight_seed"]) == ht.ESM_PORT_WEIGHT_SEED and bool(fx["fp16_matrices"])
    st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=ht.ESM_PORT_WEIGHT_SEED)
    wt, idx = ht.chains_like_the_parity_test(L, n)
    assert np.array_equal(idx, fx["idx"]) and np.array_equal(wt, fx["wt_idx"])
    assert fx["logits"].dtype == np.float64 and fx["logits"].shape == (n, L, 33) and fx["grad"].shape == (n, L, 20) and fx["score"].shape == (n,)
    P = ht.Params(st, layers, dim, heads)
    ref, half = ht.model(P, idx, F64), ht.model(P, idx, F32, half=True)
    yard = {k: m(half[k], fx[k]) for k, m in MEASURES}
    assert all(0 < y < 1e-2 for y in yard.values()), yard           # fp16 rounding, not a disagreement
    return dict(fx=fx, st=st, idx=idx, P=P, ref=ref, half=half, yard=yard)


# ---- a. golden ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_fp64_helper_is_the_port_within_a_hundredth_of_the_fp16_yardstick(geom):
    c = _case(geom)
    ratios = {}
    for k, m in MEASURES:
        d = m(c["ref"][k], c["fx"][k])
        ratios[k] = d / c["yard"][k]
        print(f"[esmport] {ht.esm_port_tag(*geom)} {k}: helper vs port {d:.3e}, yardstick {c['yard'][k]:.3e}, ratio {ratios[k]:.2e}")
    assert all(r <= PIN for r in ratios.values()), ratios


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_half_points_oracle_is_the_port_within_the_device_bound(geom):
    L, layers, dim, heads, ffn, n = geom
    c = _case(geom)
    orc = eo.EsmOracle(c["st"], layers, dim, heads, half_points=True)
    s, g = orc.score_grad(c["idx"].astype(np.int64))
    with torch.no_grad():
        x = torch.nn.functional.one_hot(torch.as_tensor(c["idx"]).long(), 20).float()
        lg = orc.logits(orc._embed_perm(x))
    ratios = {}
    for (k, m), got in zip(MEASURES, (lg, s, g)):
        ratios[k] = m(got, c["fx"][k]) / (ht.MARGIN * c["yard"][k])
        print(f"[esmport] {ht.esm_port_tag(*geom)} {k}: half-points oracle vs port = {ratios[k]:.2f} of 4 x yardstick")
    assert all(r <= 1.0 for r in ratios.values()), ratios


# ---- c. what the comparison rejects --------------------------------------------------------------------------------------
def _tanh_gelu(mp):
    mp.setattr(ht, "gelu", lambda x: 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))))


def _no_token_dropout_scale(mp):
    mp.setattr(eo, "TOKEN_DROPOUT_SCALE", 1.0)


def _rotary_from_1(mp, which):
    """Positions 1 .. T in place of 0 .. T - 1 for the tensors whose ordinal among a layer's _rotary calls (0: q, 1: k) is in `which`."""
    orig, calls = ht._rotary, [0]

    def rot(x, dtype, half, *a, **k):
        j = calls[0] % 2
        calls[0] += 1
        return orig(x, dtype, half, shift_from=0) if j in which else orig(x, dtype, half)
    mp.setattr(ht, "_rotary", rot)


def _rotary_interleaved(mp):
    def rot(x, dtype, half, *a, **k):                                 # pairs (2j, 2j + 1) rotated by angle j, GPT-J style
        T, hd = x.shape[-2], x.shape[-1]
        inv = 1.0 / (10000 ** (torch.arange(0, hd, 2).to(dtype) / hd))
        fr = torch.outer(torch.arange(T).to(dtype), inv).repeat_interleave(2, -1)
        xr = torch.stack((-x[..., 1::2], x[..., 0::2]), -1).reshape(x.shape)
        return x * fr.cos() + xr * fr.sin()
    mp.setattr(ht, "_rotary", rot)


def _q_scale_dim(mp):
    def scale_q(P, raw, half=False, mut=None):
        return torch.cat((raw[..., :P.dim] * (P.dim ** -0.5), raw[..., P.dim:]), -1)
    mp.setattr(ht, "scale_q", scale_q)


def _ln_eps_1e12(mp):
    def ln(P, x, pre, dtype, mut=None):
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), P.vec(pre + ".weight", dtype), P.vec(pre + ".bias", dtype), 1e-12)
    mp.setattr(ht, "_ln", ln)


def _no_lm_head_bias(mp):
    orig = ht.Params.vec
    mp.setattr(ht.Params, "vec", lambda self, name, dtype: orig(self, name, dtype) * (0.0 if name == "lm_head.bias" else 1.0))


def _post_ln(mp):
    """x = LN1(x + attention(x)); x = LN2(x + ffn(x)): the sublayers read the stream itself, the norms follow the residual sums."""
    def qkv_unscaled(P, i, xin, dtype=F64, half=False, mut=None):
        return torch.cat([ht._lin(P, xin.to(dtype), f"layers.{i}.self_attn.{nm}_proj", dtype, half) for nm in "qkv"], -1)

    def stage_b(P, i, xin, qkv, dtype=F64, half=False, mut=None):
        ctx = ht.attention(P, qkv, dtype, half, mut)
        return ctx, ht._ln(P, xin.to(dtype) + ht._lin(P, ctx, f"layers.{i}.self_attn.out_proj", dtype, half), f"layers.{i}.self_attn_layer_norm", dtype)

    def stage_c(P, i, xmid, dtype=F64, half=False, mut=None, gelu_grad_fp16=True):
        hdn = ht._lin(P, xmid.to(dtype), f"layers.{i}.fc1", dtype, half)
        y = xmid + ht._lin(P, ht.gelu(hdn), f"layers.{i}.fc2", dtype, half)
        return ht.gelu_grad(hdn.detach()), ht._ln(P, y, f"layers.{i}.final_layer_norm", dtype)
    mp.setattr(ht, "qkv_unscaled", qkv_unscaled)
    mp.setattr(ht, "stage_b", stage_b)
    mp.setattr(ht, "stage_c", stage_c)


FAULTS = [("tanh_gelu", _tanh_gelu), ("no_token_dropout_scale", _no_token_dropout_scale),
          ("rotary_keys_from_1", lambda mp: _rotary_from_1(mp, (1,))), ("rotary_interleaved", _rotary_interleaved),
          ("q_scale_dim", _q_scale_dim), ("ln_eps_1e12", _ln_eps_1e12), ("no_lm_head_bias", _no_lm_head_bias), ("post_ln", _post_ln)]


def _fault_ratios(geom, plant):
    """{quantity: (distance / (yardstick / 100), distance / (4 x yardstick))} of the fp64 helper with the fault planted."""
    c = _case(geom)
    with pytest.MonkeyPatch.context() as mp:
        plant(mp)
        out = ht.model(c["P"], c["idx"], F64)
    return {k: (m(out[k], c["fx"][k]) / (PIN * c["yard"][k]), m(out[k], c["fx"][k]) / (ht.MARGIN * c["yard"][k])) for k, m in MEASURES}


@pytest.mark.parametrize("geom", TWO_LAYER, ids=IDS2)
@pytest.mark.parametrize("name,plant", FAULTS, ids=[f[0] for f in FAULTS])
def test_planted_faults_land_far_outside_the_pin(name, plant, geom):
    r = _fault_ratios(geom, plant)
    print(f"[esmport-fault] {name} {ht.esm_port_tag(*geom)}: " + ", ".join(f"{k} {a:.3g} x pin = {b:.3g} x device bound" for k, (a, b) in r.items()))
    assert max(a for a, _ in r.values()) >= FAULT_CLEARS, r


@pytest.mark.parametrize("geom", TWO_LAYER, ids=IDS2)
def test_a_common_rotary_offset_is_invisible_and_the_pin_cannot_be_asked_to_see_it(geom):
    """Positions 1 .. T for queries AND keys: q_m . k_n depends on m - n alone, so logits, score and gradient are those of
    positions 0 .. T - 1 up to fp64 rounding. Stated so that nobody reads the table's rotary row as covering it."""
    r = _fault_ratios(geom, lambda mp: _rotary_from_1(mp, (0, 1)))
    assert max(a for a, _ in r.values()) <= 1.0, r                  # inside the pin, as the unmutated helper is
    c = _case(geom)
    with pytest.MonkeyPatch.context() as mp:
        _rotary_from_1(mp, (0, 1))
        out = ht.model(c["P"], c["idx"], F64)
    assert ht.row_rel(out["logits"], c["ref"]["logits"]) < 1e-12


# ---- b. live -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _live(geom, dtype=F64, fp16_matrices=True):
    hp = _hp()
    L, layers, dim, heads, ffn, n = geom
    c = _case(geom)
    port = hp.Port(c["st"], layers, dim, heads, ffn, dtype, fp16_matrices)
    return port, port.from_onehot(c["idx"])


def _hp():
    pytest.importorskip("transformers")
    import helpers_esm_port
    return helpers_esm_port


def test_name_map_is_total_and_leaves_only_rotary_table_and_contact_head():
    hp = _hp()
    for geom in (GEOMS[0], GEOMS[-1]):
        L, layers, dim, heads, ffn, n = geom
        st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=3)
        nm = hp.name_map(layers)
        assert set(nm) == set(st) and len(set(nm.values())) == len(nm)              # every key of ours, each to a parameter of its own
        port = _live(geom)[0]                                                        # (fill() asserts shapes and that all were consumed)
        assert port.unfilled == sorted(hp.UNFILLED)
        assert port.model.lm_head.decoder.weight.data_ptr() == port.model.esm.embeddings.word_embeddings.weight.data_ptr()
        cfg = port.model.config
        assert (cfg.layer_norm_eps, cfg.token_dropout, cfg.position_embedding_type, cfg.emb_layer_norm_before) == (1e-5, True, "rotary", False)
        assert cfg._attn_implementation == "eager" and not port.model.training


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_ids_path_is_the_embeds_path_and_a_fresh_evaluation_is_the_fixture(geom):
    _hp()
    c = _case(geom)
    port, o = _live(geom)
    assert torch.equal(port.from_ids(c["idx"])["logits"], o["logits"])              # confirms TOKEN_DROPOUT_SCALE and the permutation
    for k, m in MEASURES:
        d = m(o[k], c["fx"][k])
        print(f"[esmport] {ht.esm_port_tag(*geom)} {k}: regenerated vs fixture {d:.2e}")
        assert d <= 1e-9, (k, d)


def _probs(P, qkv, dtype, half):
    """The attention probabilities [n, H L, L] as helpers_transformer.attention forms them, from q|k|v (q scaled)."""
    qkv = qkv.to(dtype)
    n, L, _ = qkv.shape
    sp = lambda t: t.reshape(n, L, P.heads, P.hd).transpose(1, 2)
    q, k = (ht._rotary(sp(qkv[..., j * P.dim:(j + 1) * P.dim]), dtype, half) for j in range(2))
    p = ht._h(torch.softmax(ht._h(q @ k.transpose(-1, -2), half), -1), half)
    return p.reshape(n, P.heads * L, L)


@pytest.mark.parametrize("geom", TWO_LAYER, ids=IDS2)
def test_every_layer_input_final_norm_and_attention_probabilities_are_the_ports(geom):
    _hp()
    c = _case(geom)
    P, ref, half, layers = c["P"], c["ref"], c["half"], geom[1]
    port = _live(geom)[0]
    o = port.from_ids(c["idx"])
    assert len(o["hidden"]) == layers + 1 and len(o["attentions"]) == layers
    pairs = [(f"xin{i}", ref[f"xin{i}"], half[f"xin{i}"], o["hidden"][i]) for i in range(layers)]
    pairs.append(("LN_after(xlast)", ht._ln(P, ref["xlast"], "emb_layer_norm_after", F64),
                  ht._ln(P, half["xlast"], "emb_layer_norm_after", F32), o["hidden"][layers]))
    for i in range(layers):
        n, H, L, _ = o["attentions"][i].shape
        pairs.append((f"P{i}", _probs(P, ref[f"qkv{i}"], F64, False), _probs(P, half[f"qkv{i}"], F32, True), o["attentions"][i].reshape(n, H * L, L)))
    ratios = {}
    for name, got, hv, theirs in pairs:
        yard = ht.row_rel(hv, theirs)
        assert yard > 0, name
        ratios[name] = ht.row_rel(got, theirs) / yard
        print(f"[esmport-stage] {ht.esm_port_tag(*geom)} {name}: {ratios[name]:.2e} of the yardstick {yard:.2e}")
    assert all(r <= PIN for r in ratios.values()), ratios


@pytest.mark.parametrize("geom", TWO_LAYER, ids=IDS2)
def test_fp32_oracle_is_as_close_to_the_fp64_port_as_the_fp32_port_is(geom):
    """True fp32 matrices on both sides. Bound: 4 x the distance of the port run in fp32 from the port in fp64 -- what fp32
    costs, measured on the independent side."""
    _hp()
    L, layers, dim, heads, ffn, n = geom
    c = _case(geom)
    p64, p32 = _live(geom, F64, False)[1], _live(geom, F32, False)[1]
    orc = eo.EsmOracle(c["st"], layers, dim, heads, half_points=False)
    s, g = orc.score_grad(c["idx"].astype(np.int64))
    with torch.no_grad():
        lg = orc.logits(orc._embed_perm(torch.nn.functional.one_hot(torch.as_tensor(c["idx"]).long(), 20).float()))
    ratios = {}
    for (k, m), got in zip(MEASURES, (lg, s, g)):
        cost = m(p32[k], p64[k])
        assert cost > 0, k
        ratios[k] = m(got, p64[k]) / (ht.MARGIN * cost)
        print(f"[esmport] {ht.esm_port_tag(*geom)} {k}: fp32 oracle vs fp64 port {m(got, p64[k]):.2e}, fp32 port vs fp64 port {cost:.2e}")
    assert all(r <= 1.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("geom", TWO_LAYER, ids=IDS2)
def test_half_points_rounding_is_the_size_of_the_ports_under_autocast(geom):
    """The oracle's header says that half_points=True rounds where autocast hands an fp16 tensor on. CPU autocast's op lists
    are not CUDA's (the reference runs torch.cuda.amp.autocast), so this checks the SIZE of the rounding effect, not its
    places: the port in fp32 under torch.autocast("cpu", float16) lies about as far from its own fp64 as
    EsmOracle(half_points=True) does -- within a factor 4 either way, on the score and on the gradient."""
    _hp()
    L, layers, dim, heads, ffn, n = geom
    c = _case(geom)
    p64 = _live(geom)[1]
    auto = _live(geom, F32, True)[0].from_onehot(c["idx"], autocast=torch.float16)
    s, g = eo.EsmOracle(c["st"], layers, dim, heads, half_points=True).score_grad(c["idx"].astype(np.int64))
    for (k, m), got in (((MEASURES[1]), s), ((MEASURES[2]), g)):
        ratio = m(got, p64[k]) / m(auto[k], p64[k])
        print(f"[esmport] {ht.esm_port_tag(*geom)} {k}: half-points oracle / autocast port = {ratio:.2f}")
        assert 0.25 <= ratio <= 4.0, (k, ratio)

"""An INDEPENDENT ESM-2: the `transformers` package's port (`EsmForMaskedLM`), built from a bare `EsmConfig` and filled with
this project's synthetic weights (ppde_amd.synthetic.make_esm2_state). No checkpoint, tokenizer, model name or hub access.

The only file that imports `transformers`; import it behind `pytest.importorskip("transformers")` (tests/test_esm_port_cpu.py)
or from the fixture generator (tests/golden/make_golden.py esm_port), never from a GPU test: those read the frozen
tests/golden/esm_port_*.npz.

What the port is evaluated on, two ways:
  * `from_ids`: token ids (the Potts letters through the permutation of oracle/esm_oracle.py), with every layer's input
    (`hidden_states[i]` = our xin_i; the last entry is emb_layer_norm_after(xlast)) and attention probabilities;
  * `from_onehot`: the Potts one-hot [n, L, 20] through the permutation matrix and the embedding matmul, times
    1 - 0.15 * 0.8, handed in as `inputs_embeds` (the port applies the token-dropout rescale to ids only):
    score = sum x * log_softmax(logits) and its autograd gradient on the one-hot.

As in helpers_transformer.Params: `dtype` fp64 or fp32, `fp16_matrices` whether the matrices enter at their fp16 values.
One property of the port to know when reading small differences: it forms the rotary angles and applies the rotation in
fp32 whatever the model's dtype, so its "fp64" carries fp32 rounding of q and k (about 1e-7 relative)."""
import os

os.environ["HF_HUB_OFFLINE"] = os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
import transformers  # noqa: E402
from transformers import EsmConfig, EsmForMaskedLM  # noqa: E402

import esm_oracle as eo  # noqa: E402
from helpers_transformer import ESM_PORT_GEOMETRIES as GEOMETRIES, ESM_PORT_WEIGHT_SEED as WEIGHT_SEED, esm_port_tag as tag  # noqa: E402,F401

F64, F32 = torch.float64, torch.float32
# what of the port this project's state does not fill: neither touches the logits
UNFILLED = ("esm.rotary_embeddings.inv_freq", "esm.contact_head.regression.weight", "esm.contact_head.regression.bias")

def name_map(n_layers):
    """make_esm2_state's key -> the port's parameter name. Total: fill() asserts that every key of the state is consumed."""
    m = {"embed_tokens.weight": "esm.embeddings.word_embeddings.weight",
         "emb_layer_norm_after.weight": "esm.encoder.emb_layer_norm_after.weight",
         "emb_layer_norm_after.bias": "esm.encoder.emb_layer_norm_after.bias",
         "lm_head.dense.weight": "lm_head.dense.weight", "lm_head.dense.bias": "lm_head.dense.bias",
         "lm_head.layer_norm.weight": "lm_head.layer_norm.weight", "lm_head.layer_norm.bias": "lm_head.layer_norm.bias",
         "lm_head.bias": "lm_head.bias"}
    for i in range(n_layers):
        ours, theirs = f"layers.{i}.", f"esm.encoder.layer.{i}."
        for wb in ("weight", "bias"):
            m[ours + "self_attn.q_proj." + wb] = theirs + "attention.self.query." + wb
            m[ours + "self_attn.k_proj." + wb] = theirs + "attention.self.key." + wb
            m[ours + "self_attn.v_proj." + wb] = theirs + "attention.self.value." + wb
            m[ours + "self_attn.out_proj." + wb] = theirs + "attention.output.dense." + wb
            m[ours + "self_attn_layer_norm." + wb] = theirs + "attention.LayerNorm." + wb
            m[ours + "final_layer_norm." + wb] = theirs + "LayerNorm." + wb
            m[ours + "fc1." + wb] = theirs + "intermediate.dense." + wb
            m[ours + "fc2." + wb] = theirs + "output.dense." + wb
    return m


def config(n_layers, dim, heads, ffn):
    cfg = EsmConfig(vocab_size=33, hidden_size=dim, num_hidden_layers=n_layers, num_attention_heads=heads, intermediate_size=ffn,
                    position_embedding_type="rotary", token_dropout=True, emb_layer_norm_before=False,
                    pad_token_id=1, mask_token_id=32, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    layer_norm_eps=1e-5, max_position_embeddings=1026)          # (the port's eps default is 1e-12; the checkpoints': 1e-5)
    cfg._attn_implementation = "eager"
    return cfg


def fill(model, state, n_layers, fp16_matrices=True):
    """Copy the state into the port. -> the port's state-dict entries left unfilled (the tied decoder excepted, which is
    checked to BE the embedding). Asserts that every key of the state is consumed and lands on a tensor of its shape."""
    nm = name_map(n_layers)
    assert set(state) <= set(nm), sorted(set(state) - set(nm))
    sd = model.state_dict()
    filled = set()
    with torch.no_grad():
        for k, v in state.items():
            w = torch.as_tensor(np.asarray(v), dtype=F32)
            if fp16_matrices and w.dim() == 2:
                w = w.half().float()
            dst = sd[nm[k]]
            assert dst.shape == w.shape, (k, tuple(dst.shape), tuple(w.shape))
            dst.copy_(w)                                             # (state_dict() tensors alias the parameters)
            filled.add(nm[k])
    assert len(filled) == len(state)                                 # the map is one to one on the state's keys
    dec, emb = model.lm_head.decoder.weight, model.esm.embeddings.word_embeddings.weight
    assert dec is emb or dec.data_ptr() == emb.data_ptr(), "lm_head.decoder is not tied to the embedding"
    return sorted(set(sd) - filled - {"lm_head.decoder.weight"})


class Port:
    """state: make_esm2_state's dict. dtype F64 / F32; fp16_matrices as helpers_transformer.Params."""

    def __init__(self, state, n_layers, dim, heads, ffn, dtype=F64, fp16_matrices=True):
        self.dtype, self.n_layers, self.dim, self.heads = dtype, n_layers, dim, heads
        model = EsmForMaskedLM(config(n_layers, dim, heads, ffn))
        self.unfilled = fill(model, state, n_layers, fp16_matrices)
        self.model = model.to(dtype).eval()
        for p in self.model.parameters():
            p.requires_grad_(False)
        self.perm = torch.as_tensor(eo.potts_to_esm_index())

    def ids(self, idx):
        return self.perm[torch.as_tensor(np.asarray(idx)).long()]

    def from_ids(self, idx):
        """-> dict: logits [n, L, 33], hidden [layers + 1] x [n, L, dim], attentions [layers] x [n, H, L, L]."""
        with torch.no_grad():
            o = self.model(input_ids=self.ids(idx), output_hidden_states=True, output_attentions=True)
        return dict(logits=o.logits, hidden=list(o.hidden_states), attentions=list(o.attentions))

    def from_onehot(self, idx, autocast=None):
        """-> dict: logits, score [n], grad [n, L, 20] (all detached). autocast: a dtype to run the port under
        torch.autocast("cpu", ...)."""
        idx = torch.as_tensor(np.asarray(idx)).long()
        x = torch.nn.functional.one_hot(idx, 20).to(self.dtype).requires_grad_()
        Pm = torch.zeros(20, 33, dtype=self.dtype)
        Pm[torch.arange(20), self.perm] = 1.0
        x_esm = x @ Pm
        E = self.model.esm.embeddings.word_embeddings.weight
        emb = (x_esm @ E) * eo.TOKEN_DROPOUT_SCALE
        if autocast is not None:
            with torch.autocast("cpu", dtype=autocast):
                lg = self.model(inputs_embeds=emb).logits
            lg = lg.to(self.dtype)
        else:
            lg = self.model(inputs_embeds=emb).logits
        s = (x_esm * torch.log_softmax(lg, -1)).sum(dim=[1, 2])
        g, = torch.autograd.grad([s.sum()], [x])
        return dict(logits=lg.detach(), score=s.detach(), grad=g.detach())


def versions():
    return transformers.__version__, torch.__version__

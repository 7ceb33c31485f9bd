"""The device against an INDEPENDENT ESM-2: logits, score and gradient of one evaluation per geometry against the frozen
output of the `transformers` package's port (tests/golden/esm_port_<geometry>.npz; fp64, matrices at their fp16 values; see
tests/helpers_esm_port.py and tests/test_esm_port_cpu.py). Reads fixtures only: the package is not needed here.

The bound is 4 x yardstick (ht.MARGIN), the yardstick being the distance from the FIXTURE, in the same measure, of the CPU
evaluation that rounds to fp16 where the device does (helpers_transformer.model(P, idx, F32, half=True)). Nothing from the
device enters it. Pad columns of the logits must be exactly zero. The ratios are recorded by test_hip_parity.observed under
esmport:<geometry>:<quantity>. A failure here means the device disagrees with an implementation of ESM-2 that this project
did not write."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_transformer as ht
from helpers import load
from helpers_transformer import F32
from ppde_amd import synthetic
from test_hip_parity import observed
from test_transformer_stages_gpu import device_buffers

GEOMS = ht.ESM_PORT_GEOMETRIES


@pytest.mark.parametrize("geom", GEOMS, ids=[ht.esm_port_tag(*g) for g in GEOMS])
def test_device_logits_score_and_gradient_vs_the_independent_port(geom):
    L, layers, dim, heads, ffn, n = geom
    tag = ht.esm_port_tag(*geom)
    fx = load(f"esm_port_{tag}.npz")
    assert tuple(int(v) for v in fx["geometry"]) == geom and int(fx["weight_seed"]) == ht.ESM_PORT_WEIGHT_SEED and bool(fx["fp16_matrices"])
    P = ht.Params(synthetic.make_esm2_state(layers, dim, heads, ffn, seed=ht.ESM_PORT_WEIGHT_SEED), layers, dim, heads)
    half = ht.model(P, fx["idx"], F32, half=True)                    # the yardstick's evaluation: CPU only
    b = device_buffers(L, layers, dim, heads, ffn, n)
    assert np.array_equal(b["idx"], fx["idx"])
    assert b["logits"].shape == (n, L, 128) and not b["logits"][..., 33:].any(), "pad columns of logits"
    got = {"logits": b["logits"][..., :33], "score": b["e"].astype(np.float64) + float(b["wt_score"]), "grad": b["grad"]}
    assert got["grad"].shape == (n, L, 20) and float(b["e"][0]) == 0.0          # chain 0 is the wild type
    ratios = {}
    for k, m in (("logits", ht.row_rel), ("score", ht.score_rel), ("grad", ht.chain_rel)):
        yard = m(half[k], fx[k])
        assert yard > 0, k
        ratios[k] = observed(f"esmport:{tag}:{k}", m(torch.as_tensor(got[k]), fx[k]), ht.MARGIN * yard)
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{tag}: device distance from the independent ESM-2 over 4 x yardstick: {bad}"

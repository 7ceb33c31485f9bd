"""The transformer expert at population scale: row counts at which the persistent GEMMs (tf_gemm160, tf_gemm_nt, the opt-in
tf_gemm_big) give a workgroup a second, third, ... output tile, checked against fp64 and against small batches.

The host launches at most 512 workgroups per GEMM (256 for tf_gemm_big); each walks its XCD's run of output tiles. Below 512
tiles the loop body runs once, and every other reference-checked evaluation of the suite stays below 128 tiles. The two
geometries of helpers_transformer.POPULATIONS are about the smallest that take EVERY GEMM with N >= 256 past the cap (the
conditions are asserted on the CPU in tests/test_transformer_stages_cpu.py): P160 (tf_gemm160: N = 640 / 1920 / 1280 reach
ordinals 1 / 3 / 2) and P128 (tf_gemm_nt: N = 256 / 768 / 512 reach 1 / 4 / 2). The vocabulary GEMMs (N = 128: 210 and 370
tiles) stay at one tile per workgroup at these sizes; nothing here claims otherwise.

One evaluation with the gradient of the whole population, then
  (a) every stage of the chains helpers_transformer.select_chains picks from the walk (chain 0, the last chain, one chain
      wholly inside the tiles of every ordinal of every GEMM shape, the chain holding the first row of a workgroup's second
      tile, one straddling two XCDs' runs) against fp64 within 4 x the yardstick, exactly as test_transformer_stages_gpu
      does for two or three chains (same functions, same measures, same margin);
  (b) the same chains evaluated again three at a time: energies and gradients of ALL chains, and every readable buffer of
      the selected chains, must be the population evaluation's bits (a chain's numbers do not depend on the
      batch it sits in);
  (c) the same population under other forms of the walk, one fresh child process each: bit equality of energies and gradients.
Ratios are recorded under tfpop:<geometry>l<layers>:<stage>[:layer]."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers_transformer as ht
from test_transformer_stages_gpu import check_stages, read_buffers

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 3                               # the batch size the stage tests bound
_DEFAULT = {}                           # (geometry, layers) -> (energies, gradients) of the population evaluation in this process


def population(geom, layers):
    """-> (model, chains [n, L]) of a geometry: the wild type and mutants as in the parity test."""
    from test_transformer_gpu import _model
    L, dim, heads, ffn, n = ht.POPULATIONS[geom]
    m, wt, _, _ = _model(L, layers, dim, heads, ffn)
    wt2, idx = ht.chains_like_the_parity_test(L, n)
    assert np.array_equal(wt, wt2) and np.array_equal(idx[0], wt)
    return m, idx


def evaluate(m, idx):
    e, _, g = m.energy_grad(torch.as_tensor(np.ascontiguousarray(idx)).cuda(), 4)
    return e.cpu().numpy(), g.cpu().numpy()


def small_batches(n, selected):
    """The n chains in batches of three: the selected ones first, in as few batches as possible."""
    rest = [c for c in range(n) if c not in set(selected)]
    fill = -len(selected) % BATCH
    order = list(selected) + rest[:fill]
    with_sel = [order[i:i + BATCH] for i in range(0, len(order), BATCH)]
    rest = rest[fill:]
    return with_sel, [rest[i:i + BATCH] for i in range(0, len(rest), BATCH)]


@pytest.mark.parametrize("geom,layers", [(g, l) for g in ht.POPULATIONS for l in (2, 1)], ids=lambda v: str(v))
def test_population_stages_vs_fp64_and_small_batches_bit_for_bit(geom, layers):
    L, dim, heads, ffn, n = ht.POPULATIONS[geom]
    selected, why, missing = ht.select_chains(L, n, dim, ffn)
    assert not missing and selected[0] == 0
    m, idx = population(geom, layers)
    e, g = evaluate(m, idx)
    _DEFAULT[(geom, layers)] = (e, g)
    pop = read_buffers(m, L, layers, dim, ffn, n)                        # (whole buffers: a read starts at the buffer's first row)

    # (b) three at a time: the population's bits
    with_sel, others = small_batches(n, selected)
    assert sorted(c for b in with_sel + others for c in b) == list(range(n))
    e3, g3, differ = np.empty_like(e), np.empty_like(g), []
    for batch in with_sel:
        e3[batch], g3[batch] = evaluate(m, idx[batch])
        small = read_buffers(m, L, layers, dim, ffn, len(batch))
        for k, v in small.items():
            for j, c in enumerate(batch):
                if c in why and not np.array_equal(v[j], pop[k][c]):
                    differ.append((k, c, int((v[j] != pop[k][c]).sum())))
    for batch in others:
        e3[batch], g3[batch] = evaluate(m, idx[batch])
    wt_score = np.float64(m.transformer_wt_score)
    m.close()
    bad_e, bad_g = np.flatnonzero(e3 != e), np.flatnonzero((g3 != g).reshape(n, -1).any(1))

    # (a) the selected chains' stages against fp64
    print(f"[tfpop] {geom}l{layers}: " + "; ".join(f"chain {c}: {', '.join(why[c])}" for c in selected))
    problems = []
    try:
        check_stages(f"{geom}l{layers}", L, layers, dim, heads, ffn, dict(pop, idx=idx, e=e, grad=g, wt_score=wt_score),
                     stages=layers == 2, chains=selected, family="tfpop")
    except AssertionError as err:                                       # (reported together with what (b) found)
        problems.append(str(err))
    if not (np.isfinite(e).all() and np.isfinite(g).all()):
        problems.append("energies or gradients are not finite")
    if differ:
        problems.append(f"buffers of selected chains differ from their batch of {BATCH} (buffer, chain, elements): {differ[:20]}")
    if len(bad_e) or len(bad_g):
        problems.append(f"chains whose energy / gradient depends on the batch: {bad_e[:20]} / {bad_g[:20]}")
    assert not problems, "\n".join(problems)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import numpy as np
from test_transformer_population_gpu import evaluate, population
m, idx = population("P160", 2)
e, g = evaluate(m, idx)
np.savez(sys.argv[2], e=e, g=g)
"""

FORMS = [("one workgroup per tile", dict(PPDE_TF_160="0", PPDE_TF_PERSIST="0")),          # the walk against no walk
         ("persistent 128-tile kernel", dict(PPDE_TF_160="0")),
         ("no touch loads", dict(PPDE_TF_TOUCH="0")),
         ("256-row tiles", dict(PPDE_TF_BIG="1", PPDE_TF_160="0"))]                       # tf_gemm_big: at most 256 workgroups, rows padded to 256


@pytest.mark.parametrize("label,env", FORMS, ids=[f[0].replace(" ", "-") for f in FORMS])
def test_other_forms_of_the_walk_give_the_population_the_same_bits(label, env):
    """Two layers of P160 in a fresh child process (the switches are read once per process). The k order per output element
    is the same in every GEMM kernel, so energies and gradients of all 256 chains must be the default's bits."""
    if ("P160", 2) not in _DEFAULT:
        m, idx = population("P160", 2)
        _DEFAULT[("P160", 2)] = evaluate(m, idx)
        m.close()
    e, g = _DEFAULT[("P160", 2)]
    with tempfile.TemporaryDirectory() as d:
        script, out = os.path.join(d, "child.py"), os.path.join(d, "population.npz")
        open(script, "w").write(_CHILD)
        r = subprocess.run([sys.executable, script, REPO, out], capture_output=True, text=True, timeout=180, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got = dict(np.load(out))
    assert np.isfinite(e).all() and np.isfinite(g).all()
    bad_e, bad_g = np.flatnonzero(got["e"] != e), np.flatnonzero((got["g"] != g).reshape(len(e), -1).any(1))
    assert not len(bad_e) and not len(bad_g), f"{label}: chains whose energy / gradient differs from the default's: {bad_e[:20]} / {bad_g[:20]}"

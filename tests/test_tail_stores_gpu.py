"""What a launch writes last is what the next launch reads first: the Potts kernel's gradient columns and energy parts, the chain
kernels' state rows, T4 copies, records and histories leave with write-through stores (common.h store_wt*). A hand-off store the
next launch does not see shows as a stale letter, gradient entry or record: another draw, another accept bit, another energy.

Case 1 runs the chain of launches every way it is issued (graph replay and eager launches, re-evaluating and reusing policy) on
the toy geometry and asks for the same bits from all of them and for the oracle's run on the device's own noise. Case 2 asks the
stateless Potts evaluation for the oracle's numbers at batch sizes that fill a chain group partly and take two chain blocks.
Tolerances are those of test_hip_parity.py (its docstring: Potts energies 5e-6 * max(1, |e|), gradients 2e-6; a run's energy
history 2e-5 as test_config2_composition_against_the_oracle compares it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppde_oracle as orc
from helpers import device_noise, load, model_from_fixture, oracle_energy
from test_hip_parity import e_tol, hip_model


def test_every_way_of_issuing_a_toy_run_gives_the_oracles_run():
    """TOY24 (L = 24, run_toy24_n1.npz's geometry: a Potts window of 16 residues from residue 4, so rows, T4 copies and gradient
    columns all have residues inside and outside the window), the synthetic Potts model of the fixtures as the only expert, 16
    chains, device RNG, pas_length 2. The runs take 20 iterations, not 12: the shortest captured graph segment is 20 iterations
    long, so a 12-step run with use_graph would be launched eagerly and compare the eager path with itself; the graph runs here
    must have replayed every step."""
    from ppde_amd.sampler import Chains
    fx = load("run_toy24_n1.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    m = hip_model(J, h, i0, wt_idx, cnn, 5.0)                                  # (which = 1 below: the Potts expert alone is the energy)
    n, T, pas, Lp = 16, 20, int(fx["pas"]), J.shape[0]
    assert pas == 2 and wt_idx.shape[0] == 24
    lo, hi = int(fx["min_pos"]), int(fx["max_pos"])
    runs = {}
    for graph in (False, True):
        for reuse in (False, True):
            ch = Chains(m, n, T, pas, 0, False, lo, hi, 1, 1, reuse_grad=reuse, trace=True, random_chain=0, seed=77, use_graph=graph)
            ch.init(torch.as_tensor(np.tile(wt_idx, (n, 1))).cuda())
            ch.run(T)
            runs[graph, reuse] = (ch, ch.trace(), ch.collect(), ch.peek())
            assert ch.graph_stats()["replayed_steps"] == (T if graph else 0)
    ch, tr, res, pk = runs[False, False]
    for key, (_, tr2, res2, pk2) in runs.items():
        for k in ("flat", "accepted", "U"):
            assert np.array_equal(tr[k], tr2[k]), (key, k)
        for k in ("energy_history", "fitness_history", "best_idx", "best_energy", "best_step", "random_traj"):
            assert np.array_equal(res[k], res2[k]), (key, k)
        for k in ("idx", "energy", "accepted", "dist"):
            assert np.array_equal(pk[k], pk2[k]), (key, k)
    noise = device_noise(ch, T, pas)
    en = oracle_energy(J, h, i0, wt_idx, None, 0.0)
    ref = orc.run(en, np.tile(wt_idx.astype(np.int64), (n, 1)), wt_idx, lambda t: noise[t], T, lo, hi, pas, 0, False, trace=True)
    for t in range(T):
        U = noise[t][0].numpy()
        assert np.array_equal(tr["U"][t], U)
        for s in range(int(U.max())):
            act = s < U
            assert np.array_equal(tr["flat"][t, s][act], ref["traces"][t]["flat"][s].numpy()[act]), (t, s)
    assert np.array_equal(tr["accepted"].astype(bool), ref["accepted"].numpy())
    assert np.abs(res["energy_history"] - ref["energy_history"].numpy()).max() <= 2e-5
    assert np.array_equal(res["best_idx"], ref["best_idx"].numpy())
    assert (res["fitness_history"] == 0).all()
    assert tr["accepted"].any() and not tr["accepted"].all()                    # both branches of the accept kernel's tail ran


@pytest.fixture(scope="module")
def pabp_potts():
    fx = load("ops_pabp_lam5.npz")
    J, h, i0, wt_idx, cnn = model_from_fixture(fx)
    rng = np.random.default_rng(130)
    idx = rng.integers(0, 20, size=(130, wt_idx.shape[0])).astype(np.uint8)
    eo, _, go = oracle_energy(J, h, i0, wt_idx, None, 0.0).energy_grad(torch.as_tensor(idx.astype(np.int64)))
    return hip_model(J, h, i0, wt_idx, cnn, 5.0), idx, eo.numpy(), go.numpy()           # (evaluated with which = 1)


@pytest.mark.parametrize("n", [1, 65, 130])
def test_stateless_potts_energy_grad_vs_oracle(pabp_potts, n):
    """ppde_energy_grad (Potts only, PABP size) on the first n of 130 random sequences: one chain, a second chain group with one
    chain in it, two chain blocks. Every gradient column and every energy part is one write-through store of the Potts kernel."""
    m, idx, eo, go = pabp_potts
    e, fit, g = m.energy_grad(torch.as_tensor(idx[:n]).cuda(), 1)
    e, g = e.cpu().numpy(), g.cpu().numpy()
    assert e.shape == (n,) and g.shape == go[:n].shape
    err_e, err_g = np.abs(e - eo[:n]), np.abs(g - go[:n]).max()
    print(f"[tail stores] n = {n}: max energy error / tolerance {float((err_e / e_tol(eo[:n])).max()):.3f}, max gradient error {err_g:.3e}")
    assert (err_e <= e_tol(eo[:n])).all()
    assert err_g <= 2e-6
    assert float(fit.abs().max()) == 0.0

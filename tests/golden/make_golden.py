#!/usr/bin/env python3
"""Generate the golden fixtures in this directory by running the REFERENCE itself (PyTorch-CPU).

Run in the build container only (the reference lives at /root/reference there and never travels):

    python tests/golden/make_golden.py

What it does
  * imports `ppde.energy`, `ppde.nets`, `ppde.protein_samplers.ppde` from /root/reference, with in-memory
    stand-ins for two absent third-party modules that the path never executes (`Bio.SeqIO.parse` -> a
    10-line FASTA reader; `esm_one_hot.pretrained` -> empty module, only touched by the transformer expert);
  * writes seeded synthetic weights (ppde_amd.synthetic) in the reference's file formats to a temp dir,
    because the real potts.pkl blobs are missing from the mount;
  * calls the reference's ProteinProductOfExperts / AugmentedLinearRegression / PPDE_PAS.run on them and
    stores inputs + outputs as .npz (states are stored as residue indices);
  * while the sampler runs, records what it drew (torch.randint / torch.multinomial / torch.rand_like) and
    afterwards checks that re-drawing the noise from the same seed in the order randint -> max_u x
    exponential_ -> rand reproduces those draws bit for bit — that is what lets a noise-explicit
    implementation replay the reference's trajectories.

`python tests/golden/make_golden.py esm_port` is the one target that does not need the reference: it needs the
`transformers` package (its ESM-2 port, evaluated on seeded synthetic weights; see esm_port_cases).

The fixtures hold data only (inputs, seeds, expected outputs) — no reference code.
"""
import argparse
import contextlib
import hashlib
import io
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from ppde_amd import synthetic  # noqa: E402
from ppde_amd.encoding import read_fasta  # noqa: E402

A = 20


def install_stubs():
    bio = types.ModuleType("Bio")
    seqio = types.ModuleType("Bio.SeqIO")

    class _Rec:
        def __init__(self, i, s):
            self.id, self.seq = i, s

    def parse(fn, fmt):
        seqs, ids = read_fasta(fn, return_ids=True)
        return [_Rec(i, s) for i, s in zip(ids, seqs)]

    seqio.parse = parse
    bio.SeqIO = seqio
    sys.modules["Bio"], sys.modules["Bio.SeqIO"] = bio, seqio
    esm = types.ModuleType("esm_one_hot")
    esm.pretrained = types.ModuleType("esm_one_hot.pretrained")
    sys.modules["esm_one_hot"], sys.modules["esm_one_hot.pretrained"] = esm, esm.pretrained
    for ctor in ("esm2_t12_35M_UR50D", "esm2_t30_150M_UR50D", "esm2_t33_650M_UR50D"):
        setattr(esm.pretrained, ctor, _stub_esm2_constructor)


# --- stand-in for the absent third-party `esm_one_hot` (nets.py:11, :176-181) -------------------------------------
# The reference's transformer expert needs `pretrained.esm2_*()` -> (model, alphabet) with
#   model(x_onehot [n, L, 33])['logits'],  alphabet.tok_to_idx,  alphabet.get_batch_converter()(pairs) -> (labels, strs,
#   one-hot tokens [1, L + 2, 33] incl. <cls>/<eos>, which nets.py:186 strips).
# The stand-in serves the BUILD'S OWN ESM-2 restatement (oracle/esm_oracle.py, fp32: on the CPU `torch.cuda.amp.autocast`
# is disabled) on seeded synthetic weights, so these fixtures do not pin the ESM arithmetic (esm_port_cases below does); what they pin is the reference's
# glue around it: nets.py:193-240 (permutation, local_score, Delta against the wild type), :302-312 (PottsTransformer),
# energy.py:110-130 (minibatch loop, gradient w.r.t. the slice) and PPDE_PAS.run on top.
STUB_ESM = dict(layers=2, dim=128, heads=4, ffn=256, seed=5)


class _StubEsm2(torch.nn.Module):
    def __init__(self, orc):
        super().__init__()
        self.orc = orc

    def forward(self, x):
        return {"logits": self.orc.logits(x)}


class _StubAlphabet:
    def __init__(self, tokens):
        self.tok_to_idx = {t: i for i, t in enumerate(tokens)}

    def get_batch_converter(self):
        def convert(pairs):
            labels, strs = [p[0] for p in pairs], [p[1] for p in pairs]
            toks = [[self.tok_to_idx["<cls>"]] + [self.tok_to_idx[c] for c in s] + [self.tok_to_idx["<eos>"]] for s in strs]
            return labels, strs, torch.nn.functional.one_hot(torch.tensor(toks), len(self.tok_to_idx)).float()
        return convert


def stub_esm_oracle():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import esm_oracle as eo
    g = STUB_ESM
    st = synthetic.make_esm2_state(g["layers"], g["dim"], g["heads"], g["ffn"], seed=g["seed"])
    return eo, eo.EsmOracle(st, g["layers"], g["dim"], g["heads"], half_points=False)


def _stub_esm2_constructor():
    eo, orc = stub_esm_oracle()
    return _StubEsm2(orc), _StubAlphabet(eo.ESM_TOKENS)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ref_args(root, protein, n_chains, lamda, pas=2, nmut=0, paper=False, unsup="potts"):
    return argparse.Namespace(energy_lamda=lamda, unsupervised_expert=unsup, protein_weights=root,
                              protein=protein, n_chains=n_chains, device="cpu", ppde_pas_length=pas,
                              nmut_threshold=nmut, paper_results=paper)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def random_states(wt_idx, n, rng, max_mut):
    """Wild-type neighbourhoods (0..max_mut substitutions) plus two fully random rows."""
    L = wt_idx.shape[0]
    idx = np.tile(wt_idx, (n, 1))
    for b in range(n - 2):
        k = rng.integers(0, max_mut + 1)
        pos = rng.choice(L, size=k, replace=False)
        idx[b, pos] = rng.integers(0, A, size=k)
    idx[n - 2:] = rng.integers(0, A, size=(2, L))
    return idx.astype(np.uint8)


def to_onehot(idx):
    return torch.nn.functional.one_hot(torch.as_tensor(idx).long(), A).float()


def ops_case(root, protein, potts_seed, symmetric, lamda, n, state_seed, out):
    """Energy / fitness / gradient of the reference for a few states."""
    from ppde.energy import ProteinProductOfExperts
    from ppde.nets import AugmentedLinearRegression
    with quiet():
        en = ProteinProductOfExperts(ref_args(root, protein, n, lamda))
        alr = AugmentedLinearRegression(os.path.join(root, protein))
    wt_idx = en.wt_onehot[0].argmax(-1).numpy().astype(np.uint8)
    idx = random_states(wt_idx, n, np.random.default_rng(state_seed), 6)
    x = to_onehot(idx).requires_grad_()
    e, fit, g = en.get_energy_and_grads(x)
    with torch.no_grad():
        e2, fit2 = en.get_energy(to_onehot(idx))
        sup = en.get_supervised_expert(to_onehot(idx))
        unsup = en.get_unsupervised_expert(to_onehot(idx))
        orc = alr(to_onehot(idx))
    xs = to_onehot(idx).requires_grad_()
    gs = torch.autograd.grad([en.get_supervised_expert(xs).sum()], xs)[0]
    potts = en.unsupervised_expert
    np.savez_compressed(
        out, protein=protein, potts_seed=potts_seed, symmetric=symmetric, lamda=lamda,
        win_start=int(potts.index_list[0]), Lp=int(potts.seq_len),
        J_sha=sha(potts.J.detach().numpy()), idx=idx, wt_idx=wt_idx,
        e=e.detach().numpy(), fit=fit.detach().numpy(), grad=g.numpy(), e_nograd=e2.numpy(), fit_nograd=fit2.numpy(),
        supervised=sup.numpy(), supervised_grad=gs.numpy(), unsupervised=unsup.numpy(), wt_H=potts.wt_H.detach().numpy(),
        oracle_alr=orc.detach().numpy())
    print("wrote", out)


def tf_ops_case(root, protein, lamda, state_seed, out):
    """energy.py:97-132 with `--unsupervised_expert transformer` and `potts+transformer` over the stand-in ESM-2: e, fit,
    grad_x (which the reference takes w.r.t. the minibatch slice: no lamda * d fit/dx in it), for 70 states so that the
    minibatch loop (64 chains, energy.py:77, :113-127) runs twice."""
    from ppde.energy import ProteinProductOfExperts
    n = 70
    payload = dict(protein=protein, lamda=lamda, potts_seed=7, **{"esm_" + k: v for k, v in STUB_ESM.items()})
    for tag, unsup in (("t", "transformer"), ("pt", "potts+transformer")):
        with quiet(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            en = ProteinProductOfExperts(ref_args(root, protein, n, lamda, unsup=unsup))
            wt_idx = en.wt_onehot[0].argmax(-1).numpy().astype(np.uint8)
            idx = random_states(wt_idx, n, np.random.default_rng(state_seed), 6)
            x = to_onehot(idx).requires_grad_()
            e, fit, g = en.get_energy_and_grads(x)
            with torch.no_grad():
                e2, fit2 = en.get_energy(to_onehot(idx))
                unsup_e = en.get_unsupervised_expert(to_onehot(idx))
            tfm = en.unsupervised_expert.transformer if unsup == "potts+transformer" else en.unsupervised_expert
            # what autograd of the WHOLE energy w.r.t. x would be (not what the reference returns): kept to show the two differ
            xs = to_onehot(idx).requires_grad_()
            gs = torch.autograd.grad([en.get_supervised_expert(xs).sum()], xs)[0]
        payload.update({f"{tag}_e": e.detach().numpy(), f"{tag}_fit": fit.detach().numpy(), f"{tag}_grad": g.numpy(),
                        f"{tag}_e_nograd": e2.numpy(), f"{tag}_fit_nograd": fit2.numpy(), f"{tag}_unsupervised": unsup_e.numpy(),
                        f"{tag}_wt_score": tfm.wt_score.detach().numpy(), f"{tag}_perm": tfm.potts_to_esm_perm.numpy()})
        payload.update(idx=idx, wt_idx=wt_idx, supervised_grad=gs.numpy())
        if unsup == "potts+transformer":
            potts = en.unsupervised_expert.potts
            payload.update(win_start=int(potts.index_list[0]), Lp=int(potts.seq_len), J_sha=sha(potts.J.detach().numpy()),
                           wt_H=potts.wt_H.detach().numpy())
    np.savez_compressed(out, **payload)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def straight_through_case(root, protein, out):
    """get_energy under autograd (energy.py:97-101), fed what the relaxed-categorical baseline feeds it: straight-through
    samples `(x_soft + x_hard) - x_soft` drawn by the reference's own MALAApprox.straight_through_sample
    (mala_approx.py:18-23, :36-42) -- one-hot up to an ulp. Frozen: those inputs, (e, fit), d e.sum() / d input and the
    gradient of a weighted sum of e and fit, for the Potts product of experts and both transformer branches; and the
    gradient the baseline itself obtains w.r.t. its logits (mala_approx.py:73-75)."""
    import argparse
    from ppde.energy import ProteinProductOfExperts
    from ppde.protein_samplers.mala_approx import MALAApprox
    n, tau = 6, 0.9
    mala = MALAApprox(argparse.Namespace(diffusion_relaxation_tau=tau, diffusion_step_size=0.1))
    payload = dict(protein=protein, potts_seed=7, tau=tau, **{"esm_" + k: v for k, v in STUB_ESM.items()})
    for tag, unsup, lamda in (("p", "potts", 5.0), ("t", "transformer", 300.0), ("pt", "potts+transformer", 100.0)):
        with quiet(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            en = ProteinProductOfExperts(ref_args(root, protein, n, lamda, unsup=unsup))
            wt_idx = en.wt_onehot[0].argmax(-1).numpy().astype(np.uint8)
            idx = random_states(wt_idx, n, np.random.default_rng(41), 4)
            torch.manual_seed(77)
            x_soft = (1 - tau) * (1.0 / 20) * torch.ones(n, len(wt_idx), 20) + tau * to_onehot(idx)
            dist = torch.distributions.relaxed_categorical.RelaxedOneHotCategorical(torch.tensor([tau]), probs=x_soft)
            logits = dist.logits.detach().requires_grad_()
            dist = torch.distributions.relaxed_categorical.RelaxedOneHotCategorical(torch.tensor([tau]), logits=logits)
            x_st = mala.straight_through_sample(dist)
            e_chain, _ = en.get_energy(x_st)
            logit_grad = torch.autograd.grad([e_chain.sum()], [logits])[0]
            leaf = x_st.detach().clone().requires_grad_()
            e, fit = en.get_energy(leaf)
            g_e = torch.autograd.grad([e.sum()], [leaf], retain_graph=True)[0]
            w_e, w_f = torch.rand(n) + 0.5, torch.rand(n) - 0.5
            g_mix = torch.autograd.grad([(w_e * e + w_f * fit).sum()], [leaf])[0]
        payload.update({f"{tag}_lamda": lamda, f"{tag}_x": leaf.detach().numpy(), f"{tag}_e": e.detach().numpy(),
                        f"{tag}_fit": fit.detach().numpy(), f"{tag}_grad_e": g_e.numpy(), f"{tag}_w_e": w_e.numpy(),
                        f"{tag}_w_fit": w_f.numpy(), f"{tag}_grad_mix": g_mix.numpy(),
                        f"{tag}_baseline_logit_grad_absmax": float(logit_grad.abs().max())})
        payload.update(wt_idx=wt_idx)
        if unsup == "potts":
            potts = en.unsupervised_expert
            payload.update(win_start=int(potts.index_list[0]), Lp=int(potts.seq_len), J_sha=sha(potts.J.detach().numpy()))
        print(f"  {unsup}: max |x - one-hot| {float((leaf.detach() - leaf.detach().round()).abs().max()):.2e}, "
              f"|d e / d logits| of the baseline {float(logit_grad.abs().max()):.2e}, max |d e / d x| {float(g_e.abs().max()):.3f}")
    np.savez_compressed(out, **payload)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def file_sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def real_case(protein, lamda, n, state_seed, out):
    """The reference on the REAL shipped supervised / ground-truth weights (weights/<protein>/onehot_cnn_seed=*.pt,
    results-...-linear.pkl, wt.fasta) next to a synthetic potts.pkl (the real one is a missing blob). The fixture
    holds the files' SHA-256, the states and the reference's outputs: no weight values."""
    src = os.path.join("/root/reference/weights", protein)
    with tempfile.TemporaryDirectory() as root:
        d = synthetic.write_weights_dir(root, protein, potts_seed=1234, cnn_seeds=(), linear_seeds=())
        real_wt = read_fasta(os.path.join(src, "wt.fasta"), return_ids=True)
        assert real_wt == read_fasta(os.path.join(d, "wt.fasta"), return_ids=True), "synthetic.PROTEINS differs from the shipped wt.fasta"
        names = sorted(f for f in os.listdir(src) if f.endswith(".pt") or f.endswith("-linear.pkl"))
        for f in names:
            os.symlink(os.path.join(src, f), os.path.join(d, f))
        tmp = out + ".tmp.npz"
        ops_case(root, protein, 1234, True, lamda, n, state_seed, tmp)
        fx = dict(np.load(tmp))
        os.remove(tmp)
    fx["files"] = np.array(names + ["wt.fasta"])
    fx["file_sha"] = np.array([file_sha(os.path.join(src, f)) for f in names + ["wt.fasta"]])
    np.savez_compressed(out, **fx)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def real_cnn_weights(protein, out):
    """The VALUES of the shipped supervised-CNN checkpoints of one protein (weights/<protein>/onehot_cnn_seed={0,1,2}.pt,
    data files, 340 kB for PABP) as a fixture, so that the GPU box -- which never sees /root/reference -- can run the
    HIP CNN kernel on TRAINED weights against what the reference computed from them (real_<protein>.npz)."""
    from ppde_amd.weights import load_cnn_states
    src = os.path.join("/root/reference/weights", protein)
    states = load_cnn_states(src)
    payload = {f"net{k}.{name}": v for k, sd in enumerate(states) for name, v in sd.items()}
    payload["file_sha"] = np.array([file_sha(os.path.join(src, f"onehot_cnn_seed={k}.pt")) for k in range(len(states))])
    np.savez_compressed(out, **payload)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def real_linear_weights(protein, out):
    """The VALUES of the shipped ground-truth ridge models of one protein (weights/<protein>/results-...-seed={0..19}-linear.pkl,
    data files: a dict of coef_, intercept_, reg_coef each) with the files' SHA-256, so that the loader test on the shipped
    weights (test_oracle_golden.py::test_real_shipped_weights) runs from the repository alone."""
    import pickle
    import ppde
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(ppde.__file__))), "weights", protein)
    payload, names = {}, []
    for s in range(20):
        name = f"results-predictor=ev+onehot-train=-1-seed={s}-linear.pkl"
        with open(os.path.join(src, name), "rb") as fh:
            d = pickle.load(fh)
        assert sorted(d) == ["coef_", "intercept_", "reg_coef"], sorted(d)
        payload[f"seed{s}.coef_"] = np.asarray(d["coef_"])
        payload[f"seed{s}.intercept_"] = np.asarray(d["intercept_"])
        payload[f"seed{s}.reg_coef"] = np.asarray(d["reg_coef"])
        names.append(name)
    payload["files"] = np.array(names)
    payload["file_sha"] = np.array([file_sha(os.path.join(src, f)) for f in names])
    np.savez_compressed(out, **payload)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def run_case(root, protein, lamda, n, T, seed, pas, nmut, paper, out, store_q, unsup="potts"):
    """One reference sampler run with everything it drew recorded. unsup = 'transformer' / 'potts+transformer': the
    reference's energy.py:110-130 branch over the stand-in ESM-2 (see install_stubs)."""
    from ppde.energy import ProteinProductOfExperts
    from ppde.nets import AugmentedLinearRegression
    from ppde.protein_samplers.ppde import PPDE_PAS
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import ppde_oracle as orc

    args = ref_args(root, protein, n, lamda, pas, nmut, paper, unsup)
    with quiet(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        en = ProteinProductOfExperts(args)
        alr = AugmentedLinearRegression(os.path.join(root, protein))
    L = en.wt_onehot.shape[1]
    x0 = en.wt_onehot.repeat(n, 1, 1)
    min_pos, max_pos = int(alr.potts.index_list[0]), int(alr.potts.index_list[-1])

    rec = dict(U=[], flat=[], u=[])
    o_randint, o_multinomial, o_rand_like = torch.randint, torch.multinomial, torch.rand_like

    def w_randint(*a, **k):
        r = o_randint(*a, **k)
        rec["U"].append(r.reshape(-1).clone())
        rec["flat"].append([])
        return r

    def w_multinomial(*a, **k):
        r = o_multinomial(*a, **k)
        rec["flat"][-1].append(r.reshape(-1).clone())
        return r

    def w_rand_like(*a, **k):
        r = o_rand_like(*a, **k)
        rec["u"].append(r.clone())
        return r

    def ref_run(copy_on_cpu):
        """copy_on_cpu=False: the reference exactly as it runs with --device cpu, where `cur_x.cpu().numpy()`
        ALIASES cur_x, so the in-place mutation-cap reset (ppde.py:153) also rewrites the state just recorded
        in all_x / random_traj. copy_on_cpu=True: `.cpu()` returns a copy, which is what it does for a tensor on
        the reference's default device (cuda) — the recorded state is then the one before the reset."""
        for k in rec:
            rec[k].clear()
        o_cpu = torch.Tensor.cpu
        if copy_on_cpu:
            torch.Tensor.cpu = lambda self, *a, **k: o_cpu(self, *a, **k).clone()
        np.random.seed(seed)
        torch.manual_seed(seed)
        torch.randint, torch.multinomial, torch.rand_like = w_randint, w_multinomial, w_rand_like
        try:
            with quiet(), warnings.catch_warnings():
                warnings.simplefilter("ignore")           # (torch.cuda.amp.autocast without CUDA warns once per call)
                return PPDE_PAS(args).run(x0, T, en, min_pos, max_pos, alr, log_every=10)
        finally:
            torch.randint, torch.multinomial, torch.rand_like = o_randint, o_multinomial, o_rand_like
            torch.Tensor.cpu = o_cpu

    alias = ref_run(copy_on_cpu=False)
    best_x, best_e, best_f, e_hist, f_hist, rtraj = ref_run(copy_on_cpu=True)
    for a_, b_ in zip(alias[1:5], (best_e, best_f, e_hist, f_hist)):
        assert np.array_equal(a_, b_)          # only the recorded STATES differ between the two
    np.random.seed(seed)
    random_idx = np.random.randint(0, n)

    # replay the noise stream from the seed and check it is what the reference consumed
    torch.manual_seed(seed)
    noise = [orc.draw_noise_torch(n, L * A, pas) for _ in range(T)]
    mu_max = 2 * pas - 1
    flat = -np.ones((T, mu_max, n), dtype=np.int64)
    for t in range(T):
        U, q, u = noise[t]
        assert torch.equal(U, rec["U"][t]), "randint stream mismatch"
        assert torch.equal(u, rec["u"][t]), "rand stream mismatch"
        assert len(rec["flat"][t]) == int(U.max())
        for s, f in enumerate(rec["flat"][t]):
            flat[t, s] = f.numpy()

    # pin the oracle on this trajectory right here (the CPU test repeats it from the fixture)
    potts = {"potts": en.unsupervised_expert, "potts+transformer": getattr(en.unsupervised_expert, "potts", None)}.get(unsup, alr.potts)
    wt_idx = en.wt_onehot[0].argmax(-1)
    P = orc.PottsOracle(potts.J.detach(), potts.bias.detach(), potts.index_list[0], wt_idx)
    C = orc.CnnOracle([{k: v.detach().numpy() for k, v in s.state_dict().items()} for s in en.supervised_expert.surrogates])
    if unsup == "potts":
        eo = orc.EnergyOracle(P, C, lamda)
    else:
        esm_mod, esm_orc = stub_esm_oracle()
        eo = orc.EnergyOracle(P if unsup == "potts+transformer" else None, C, lamda,
                              tf=esm_mod.TransformerDelta(esm_orc, wt_idx.numpy(), chunk=min(n, 64)))
    res = orc.run(eo, x0.argmax(-1), wt_idx, lambda t: noise[t], T, min_pos, max_pos, pas, nmut, paper, trace=True)
    res_alias = orc.run(eo, x0.argmax(-1), wt_idx, lambda t: noise[t], T, min_pos, max_pos, pas, nmut, paper,
                        record_after_reset=True)
    assert np.array_equal(res_alias["best_idx"].numpy(), alias[0].argmax(-1).numpy()), "oracle best state (cpu alias)"
    for t in range(T):
        mu = int(noise[t][0].max())
        assert np.array_equal(res["traces"][t]["flat"].numpy(), flat[t, :mu]), f"oracle draw mismatch at iter {t}"
    assert np.array_equal(res["best_idx"].numpy(), best_x.argmax(-1).numpy()), "oracle best state mismatch"
    if unsup != "potts":      # the fixture must discriminate: with lamda * d fit/dx in the proposal gradient the draws differ
        eo_full = orc.EnergyOracle(eo.potts, C, lamda, tf=eo.tf, full_grad=True)
        res_full = orc.run(eo_full, x0.argmax(-1), wt_idx, lambda t: noise[t], T, min_pos, max_pos, pas, nmut, paper, trace=True)
        n_diff = sum(int((res_full["traces"][t]["flat"].numpy() != flat[t, :int(noise[t][0].max())]).sum()) for t in range(T))
        assert n_diff > 0, "fixture cannot tell the reference's gradient from the full gradient"
        print(f"  full-gradient oracle differs from the reference in {n_diff} draws (as it must)")
    err = np.abs(res["energy_history"].numpy() - e_hist).max()
    assert err < 1e-4, err
    print(f"  oracle vs reference on this run: draws exact, best states exact, max |dE| = {err:.2e}")

    payload = dict(
        protein=protein, lamda=lamda, n=n, T=T, seed=seed, pas=pas, nmut=nmut, paper=paper,
        min_pos=min_pos, max_pos=max_pos, win_start=int(potts.index_list[0]), Lp=int(potts.seq_len),
        J_sha=sha(potts.J.detach().numpy()),
        U=np.stack([x.numpy() for x in rec["U"]]), u=np.stack([x.numpy() for x in rec["u"]]), flat=flat,
        q_sum=np.array([float(noise[t][1].double().sum()) for t in range(T)]),
        accepted=res["accepted"].numpy(),  # == reference's accept decisions (states/energies above are exact)
        energy_history=e_hist, fitness_history=f_hist, best_idx=best_x.argmax(-1).numpy().astype(np.uint8),
        best_energy=best_e, best_fitness=best_f, random_idx=random_idx,
        random_traj=np.stack([r.argmax(-1) for r in rtraj]).astype(np.uint8),
        best_idx_cpu_alias=alias[0].argmax(-1).numpy().astype(np.uint8),
        random_traj_cpu_alias=np.stack([r.argmax(-1) for r in alias[5]]).astype(np.uint8),
        oracle_best=alr(best_x).detach().numpy())
    if unsup != "potts":
        payload.update(unsup=unsup, potts_seed=7, **{"esm_" + k: v for k, v in STUB_ESM.items()})
    if store_q:
        payload["q"] = np.concatenate([noise[t][1].numpy() for t in range(T)], 0)  # [sum max_u, n, N]
    np.savez_compressed(out, **payload)
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB)")


def single_chain_case(root):
    """The reference's single-chain contract (ppde.py:178-183 special-cases n_chains == 1; nets.py:442 squeezes the ensemble
    output to a scalar): fitness_history comes back 1-D (T+1,), energy_history stays (T+1, 1), best_x [1, L, 20]."""
    out = os.path.join(HERE, "run_toy24_n1.npz")
    run_case(root, "TOY24", 5.0, 1, 20, 120, 2, 3, False, out, store_q=True)
    fx = np.load(out)
    assert fx["fitness_history"].shape == (21,) and fx["energy_history"].shape == (21, 1) and fx["best_fitness"].shape == (1,)


def script_case(root, protein, n_chains, n_iters, seed, out):
    """The reference's own command line (BASELINE.json configs[0]): scripts/directed_evolution.py end to end."""
    import glob
    import runpy
    sys.modules.setdefault("cma", types.ModuleType("cma"))          # imported by a baseline sampler, never used here
    res = tempfile.mkdtemp()
    argv = ["directed_evolution.py", "--protein_weights", root, "--protein", protein, "--results_path", res,
            "--hub_dir", res, "--device", "cpu", "--disable_MSA_transformer_scoring", "--sampler", "PPDE",
            "--unsupervised_expert", "potts", "--n_chains", str(n_chains), "--n_iters", str(n_iters),
            "--seed", str(seed), "--log_every", "50"]
    old = sys.argv
    sys.argv = argv
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            runpy.run_path("/root/reference/scripts/directed_evolution.py", run_name="__main__")
    finally:
        sys.argv = old
    d = glob.glob(os.path.join(res, protein, "*"))[0]
    ld = lambda f: np.load(os.path.join(d, f))
    log = [l for l in buf.getvalue().splitlines() if l.startswith("[Iteration") or l.startswith("WT protein")]
    np.savez_compressed(
        out, protein=protein, n=n_chains, T=n_iters, seed=seed, argv=np.array(argv[1:]),
        population=ld("population.npy").argmax(-1).astype(np.uint8), pred_fitness=ld("pred_fitness_scores.npy"),
        oracle_fitness=ld("oracle_fitness_scores.npy"), potts_scores=ld("potts_scores.npy"),
        energy_scores=ld("energy_scores.npy"), energy_history=ld("energy_history.npy"),
        fitness_history=ld("fitness_history.npy"), log=np.array(log))
    print("wrote", out, f"({os.path.getsize(out) / 1e3:.0f} kB); reference log head:", log[:2])


def esm_port_cases(only_check=False):
    """The `transformers` package's ESM-2 port (tests/helpers_esm_port.py: built from a bare config, filled with the seeded
    synthetic weights, fp64, matrices at their fp16 values) on the inputs of tests/test_transformer_stages_gpu.py: logits,
    score and the gradient on the Potts one-hot, one file per geometry. Needs neither the reference nor any download."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import helpers_esm_port as hp
    import helpers_transformer as ht
    tv, pv = hp.versions()
    for geom in hp.GEOMETRIES:
        L, layers, dim, heads, ffn, n = geom
        st = synthetic.make_esm2_state(layers, dim, heads, ffn, seed=hp.WEIGHT_SEED)
        wt, idx = ht.chains_like_the_parity_test(L, n)
        port = hp.Port(st, layers, dim, heads, ffn, hp.F64, fp16_matrices=True)
        assert port.unfilled == sorted(hp.UNFILLED), port.unfilled
        o = port.from_onehot(idx)
        assert torch.equal(o["logits"], port.from_ids(idx)["logits"]), "ids path differs from the embeds path"
        out = os.path.join(HERE, f"esm_port_{hp.tag(*geom)}.npz")
        np.savez_compressed(out, idx=idx.astype(np.uint8), wt_idx=wt, geometry=np.array(geom, np.int64), weight_seed=hp.WEIGHT_SEED,
                            fp16_matrices=True, logits=o["logits"].numpy(), score=o["score"].numpy(), grad=o["grad"].numpy(),
                            transformers_version=tv, torch_version=pv)
        kb = os.path.getsize(out) / 1e3
        assert kb < 300, (out, kb)
        print("wrote", out, f"({kb:.0f} kB)")


def main():
    if "esm_port" in sys.argv[1:]:
        torch.set_num_threads(1)
        esm_port_cases()
        return
    if not os.path.isdir("/root/reference/ppde"):
        sys.exit("the reference is not mounted here; fixtures can only be regenerated in the build container")
    sys.path.insert(0, "/root/reference")
    install_stubs()
    only = sys.argv[1:]
    torch.set_num_threads(1)  # reference CPU path is bit-stable at a fixed thread count
    if only and "real" in only:
        # lamda per protein as the reference's README recommends for the Potts expert (README.md:65-69)
        for protein, lam, seed in (("PABP_YEAST_Fields2013", 5.0, 21), ("UBE4B_MOUSE_Klevit2013-nscor_log2_ratio", 0.5, 22),
                                   ("GFP_AEQVI_Sarkisyan2016", 15.0, 23)):
            real_case(protein, lam, 6, seed, os.path.join(HERE, f"real_{protein.split('_')[0].lower()}.npz"))
        return
    if only and "realcnn" in only:
        # the values of the shipped checkpoints of all three proteins (PABP 0.34, UBE4B 0.4, GFP 1.6 MB): UBE4B and GFP take the
        # chunked HIP kernels, and they are the supervised expert of BASELINE configs 5 and 4
        for protein in ("PABP_YEAST_Fields2013", "UBE4B_MOUSE_Klevit2013-nscor_log2_ratio", "GFP_AEQVI_Sarkisyan2016"):
            real_cnn_weights(protein, os.path.join(HERE, f"real_{protein.split('_')[0].lower()}_cnn.npz"))
        return
    if only and "reallinear" in only:
        for protein in ("PABP_YEAST_Fields2013", "UBE4B_MOUSE_Klevit2013-nscor_log2_ratio", "GFP_AEQVI_Sarkisyan2016"):
            real_linear_weights(protein, os.path.join(HERE, f"real_{protein.split('_')[0].lower()}_linear.npz"))
        return
    if only and "single" in only:
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
            single_chain_case(root)
        return
    if only and "tf" in only:
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
            # lamda is far above the README's 1-5 on purpose: the synthetic CNN's input gradient is ~1e-2 against ~1e1 for
            # the stand-in transformer's, and the fixtures must tell "lamda * d fit/dx is in grad_x" from "it is not" well
            # above the fp16 tolerance of the GPU tests (run_case asserts that the full-gradient oracle does NOT replay)
            tf_ops_case(root, "TOY24", 300.0, 31, os.path.join(HERE, "ops_tfpoe_toy.npz"))
            # 72 chains: the reference's minibatch loop runs twice per evaluation (64 + 8)
            run_case(root, "TOY24", 300.0, 72, 10, 301, 2, 3, False, os.path.join(HERE, "run_tfpoe_toy_t.npz"), store_q=False,
                     unsup="transformer")
            run_case(root, "TOY24", 100.0, 8, 20, 302, 2, 0, False, os.path.join(HERE, "run_tfpoe_toy_pt.npz"), store_q=False,
                     unsup="potts+transformer")
        return
    if only and "straight" in only:
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
            straight_through_case(root, "TOY24", os.path.join(HERE, "ops_straight_through_toy.npz"))
        return
    if only and "script" in only:
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_weights_dir(root, "PABP_YEAST_Fields2013", potts_seed=1234)
            torch.set_num_threads(8)
            script_case(root, "PABP_YEAST_Fields2013", 16, 100, 7, os.path.join(HERE, "script_pabp_config1.npz"))
        return
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "TOY24", potts_seed=7)
        synthetic.write_weights_dir(root, "PABP_YEAST_Fields2013", potts_seed=1234)
        ops_case(root, "TOY24", 7, True, 5.0, 8, 11, os.path.join(HERE, "ops_toy24_lam5.npz"))
        ops_case(root, "PABP_YEAST_Fields2013", 1234, True, 5.0, 8, 12, os.path.join(HERE, "ops_pabp_lam5.npz"))
        ops_case(root, "PABP_YEAST_Fields2013", 1234, True, 0.0, 8, 13, os.path.join(HERE, "ops_pabp_lam0.npz"))
        # trajectories with the exponential variates stored (toy size)
        for tag, pas, nmut, paper, lam in [("a", 2, 0, False, 5.0), ("b", 1, 3, False, 5.0),
                                           ("c", 3, 2, True, 0.0), ("d", 2, 3, False, 0.0)]:
            run_case(root, "TOY24", lam, 8, 20, 100 + ord(tag), pas, nmut, paper,
                     os.path.join(HERE, f"run_toy24_{tag}.npz"), store_q=True)
        single_chain_case(root)
        # PABP-size trajectories: noise is re-drawn from the seed by the test (q_sum guards the stream)
        k = 0
        for paper in (False, True):
            for nmut in (0, 3):
                for pas in (1, 2, 5):
                    k += 1
                    run_case(root, "PABP_YEAST_Fields2013", 5.0 if k % 2 else 0.0, 16, 30, 1000 + k, pas, nmut, paper,
                             os.path.join(HERE, f"run_pabp_{k:02d}.npz"), store_q=False)
    with tempfile.TemporaryDirectory() as root:
        # couplings that are NOT symmetric: autograd still yields the symmetrised gradient
        synthetic.write_weights_dir(root, "TOY24", potts_seed=8, symmetric=False)
        ops_case(root, "TOY24", 8, False, 5.0, 8, 14, os.path.join(HERE, "ops_toy24_nonsym.npz"))
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_weights_dir(root, "PABP_YEAST_Fields2013", potts_seed=1234)
        torch.set_num_threads(8)
        script_case(root, "PABP_YEAST_Fields2013", 16, 100, 7, os.path.join(HERE, "script_pabp_config1.npz"))


if __name__ == "__main__":
    main()

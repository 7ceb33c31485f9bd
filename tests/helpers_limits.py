"""The C ABI's declared shape limits (include/ppde_hip.h, "Shape limits") at their edges: fp64 references of the two experts
in plain numpy, and the ONE table of named cases that tests/test_abi_limits_cpu.py (fp32 oracle against fp64, no GPU) and
tests/test_abi_limits_gpu.py (the library against fp64) both read, so that both see the same inputs.

Nothing here calls a project kernel or an oracle class: the fp64 code is the third, independent statement of the operations.

Tolerances (SURVEY.md section 8(c) as applied in tests/test_hip_shapes.py, now against fp64):
    energy    5e-6 max(1, |e|) + 4e-6 lamda max(1, |fit|)
    fitness   5e-6 max(1, |fit|)
    gradient  2e-6 max(1, lamda) max(1, max |g|)
They hold as they are at the reference's shape (C = L, F = 2L, K = 5, L <= 307). Elsewhere nobody has measured what fp32 itself
costs, so the budget of a quantity is max(project tolerance, 4 x err32), err32 = the fp32 ORACLE's own distance from fp64 on the
same inputs (the largest over the case's chains), computed on the CPU: x2 for another summation order, x2 for the documented
3 * 2^-22 per split-precision product on top of fp32 accumulation. No number comes from the device.
"""
import functools

import numpy as np

from helpers import _cnn_fp64, cnn_grad_decompose
from ppde_amd import synthetic

A = 20


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------
def potts_fp64(J, h, i0, wt, idx, with_H=False):
    """(dH [n], grad [n, L, 20]) of states idx [n, L] in fp64: window x_w = x[i0 : i0 + Lp], M = (J + J^T) / 2 over flattened
    (residue, letter) pairs (include/ppde_hip.h, ppde_model_set_potts), H = 1/2 x_w M x_w + h x_w, dH = H(x) - H(wt),
    grad = M x_w + h inside the window and 0 outside (sign and normalisation of oracle/ppde_oracle.py PottsOracle, which is
    pinned to the reference's fixtures). J is read in row blocks: no fp64 copy of the couplings is formed. with_H: also H(wt)."""
    J, h = np.asarray(J), np.asarray(h, dtype=np.float64)
    Lp, Np = J.shape[0], J.shape[0] * A
    idx, wt = np.asarray(idx).astype(np.int64), np.asarray(wt).astype(np.int64).reshape(1, -1)
    n, L = idx.shape
    rows = np.concatenate([wt, idx], 0)[:, i0:i0 + Lp]                                   # the wild type first
    X = np.zeros((n + 1, Np))
    X[np.arange(n + 1)[:, None], np.arange(Lp)[None, :] * A + rows] = 1.0
    Jm = np.ascontiguousarray(J.transpose(0, 2, 1, 3)).reshape(Np, Np)                  # rows (i, k), columns (j, l); fp32 as given
    Mx = np.zeros((n + 1, Np))
    for lo in range(0, Np, 1024):
        hi = min(Np, lo + 1024)
        S = Jm[lo:hi].astype(np.float64) + Jm[:, lo:hi].T.astype(np.float64)           # 2 M[lo:hi, :]
        Mx[:, lo:hi] = 0.5 * (X @ S.T)
    hf = h.reshape(Np)
    H = 0.5 * (X * Mx).sum(1) + X @ hf
    grad = np.zeros((n, L, A))
    grad[:, i0:i0 + Lp] = (Mx[1:] + hf).reshape(n, Lp, A)
    if with_H:
        return H[1:] - H[0], grad, H[0]
    return H[1:] - H[0], grad


def cnn_fp64(states, idx):
    """(fit [n], grad [n, L, 20]) of the supervised ensemble in fp64 for any number of networks, C, K, F: fit = mean over the
    networks of  wd . max_t relu(We relu(conv(x)) + be) + bd;  the arg-max over the rows t takes the FIRST row on exact ties
    (numpy's argmax) and the gradient is routed through it (features whose maximum is 0 route nothing). The weights in fp64
    and their layout are helpers._cnn_fp64's; the forward pass runs over all chains at once."""
    idx = np.asarray(idx).astype(np.int64)
    n, L = idx.shape
    fit, grad = np.zeros(n), np.zeros((n, L, A))
    for sd in states:
        _, _, _, Wflat, We, wd, K = _cnn_fp64(sd, idx[0])                                # Wflat [(kappa, a), C], We [F, C], wd [F]
        b1, b2, bd = (np.asarray(sd[k], dtype=np.float64).reshape(-1) for k in ("encoder.bias", "embedding.0.bias", "decoder.bias"))
        T = L - K + 1
        pre1 = b1 + sum(Wflat[kappa * A + idx[:, kappa:kappa + T]] for kappa in range(K))   # [n, T, C]: a one-hot window picks rows
        h1 = np.maximum(pre1, 0.0)
        h2 = np.maximum(h1 @ We.T + b2, 0.0)                                             # [n, T, F]
        top, first = h2.max(1), h2.argmax(1)                                             # [n, F]
        fit += top @ wd + bd[0]
        for b in range(n):
            pos = np.nonzero(top[b] > 0)[0]
            D = np.zeros((T, We.shape[1]))
            np.add.at(D, first[b, pos], wd[pos, None] * We[pos])
            D *= h1[b] > 0
            dwin = (D @ Wflat.T).reshape(T, K, A)
            for kappa in range(K):
                grad[b, kappa:kappa + T] += dwin[:, kappa]
    return fit / len(states), grad / len(states)


def case_is_tie_free(states, idx, gap=5e-6):
    """True when the fp64 first-row routing is the only admissible one for every chain: every group of
    helpers.cnn_grad_decompose is an EXACT arg-max tie (identical K-mers: every implementation computes the same bits for the
    tied rows and must take the first) and there is no ReLU kink. Near-ties and kinks make the routed gradient
    implementation-defined; such inputs are not used here, so no chain is ever exempted. (A kink on a row that is itself a
    candidate of a tie makes no group: cnn_grad_decompose reports it as `unresolved`, which without the rank means exactly that.)"""
    for row in np.asarray(idx):
        dec = cnn_grad_decompose(states, row, gap, want_rank=False)
        if dec["unresolved"] or any(i[0] == "kink" for i in dec["info"]) or not all(dec["exact"]):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_cnn(C, K, F, seed):
    """numpy state dict of one OnehotCNN with C channels, K taps and F features (the reference ties C = L, F = 2L; the ABI does
    not), U(-1/sqrt(fan_in), +) like torch's defaults and synthetic.make_cnn_state."""
    rng = np.random.default_rng(20_000 + seed)

    def u(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return rng.uniform(-b, b, size=shape).astype(np.float32)

    return {"encoder.weight": u((C, A, K), A * K), "encoder.bias": u((C,), A * K), "embedding.0.weight": u((F, C), C),
            "embedding.0.bias": u((F,), C), "decoder.weight": u((1, F), F), "decoder.bias": u((1,), F)}


def make_rows(wt, n, rng, forced=(), span=None):
    """n chains: the wild type, lightly mutated rows (1 + b % 16 residues of `span` (default: all) set to another letter, plus the
    `forced` residues on odd rows), and one fully random row last."""
    L = wt.shape[0]
    lo, hi = span or (0, L)
    idx = np.tile(wt, (n, 1))
    for b in range(1, n - 1):
        pos = lo + rng.choice(hi - lo, size=min(hi - lo, 1 + b % 16), replace=False)
        idx[b, pos] = (wt[pos] + rng.integers(1, A, len(pos))) % A if span else rng.integers(0, A, len(pos))
        if b % 2 == 1:
            for p in forced:
                idx[b, p] = (wt[p] + 1 + (p + b) % 19) % A
    if n > 1:
        idx[n - 1] = rng.integers(0, A, L)
    return idx.astype(np.uint8)


def chunk_edge_residues(L, K):
    """residues whose change moves the first and last K-mers and the rows on both sides of the first 64-row forward chunk
    boundary (rows 63 | 64, when the sequence has them)"""
    out = list(range(K)) + list(range(L - K, L))
    if L - K + 1 > 64:
        out += [62, 63, 64, 65]
    return sorted(set(p for p in out if 0 <= p < L))


# ---------------------------------------------------------------------------------------------------------------------
# the case table. `form` is the launch form the host code (ppde_amd/csrc/ppde_api.hip) takes for the case, derived by hand from
# cnn_single_launch (chunked when rows(T) > 128, FP > 512, or twice the single-launch LDS exceeds 160 KiB), cnn_parts (the last
# network cut in two when single launch, n_nets <= 3 and FP >= 32) and launch_experts_fused (which = 3, single launch, K = 5).
# CP = C rounded up to 32, FP = F to 16, rows(T) = T = L - K + 1 rounded up to 16; KT = 5 for K = 5, else the 8-tap tables.
# ---------------------------------------------------------------------------------------------------------------------
def _cnn(name, L, C, K, F, nets=3, n=4, potts=None, seed=0, form=""):
    return dict(name=name, L=L, C=C, K=K, F=F, nets=nets, n=n, potts=potts, seed=seed, form=form)


CNN_CASES = [
    # ---- n_nets in {1, 2, 4} at the PABP shape, with the Potts window: k_experts (fused), 6 row tiles -------------------------
    # The PABP pin of launch_experts_fused asks for n_nets == 3 && n_parts == 4 next to the shape: none of these may take it.
    # n = 70: potts_ng_for(70) = 2 chain groups (and the pin's NG == 2 holds, so only the network count keeps it away).
    _cnn("pabp_nets1", 96, 96, 5, 192, nets=1, n=6, potts=(80, 8), form="fused k_experts<6, NG 1>, 2 parts (1 network cut in two)"),
    _cnn("pabp_nets2", 96, 96, 5, 192, nets=2, n=6, potts=(80, 8), form="fused k_experts<6, NG 1>, 3 parts"),
    _cnn("pabp_nets4", 96, 96, 5, 192, nets=4, n=6, potts=(80, 8),
         form="fused k_experts<6, NG 1>, 4 parts = 4 WHOLE networks (n_nets <= 3 fails: no cut); cnn_ni == 4 reorders the units as if one were a half"),
    _cnn("pabp_nets1_n70", 96, 96, 5, 192, nets=1, n=70, potts=(80, 8), form="fused k_experts<6, NG 2>, 2 parts, two chain groups"),
    _cnn("pabp_nets2_n70", 96, 96, 5, 192, nets=2, n=70, potts=(80, 8), form="fused k_experts<6, NG 2>, 3 parts, two chain groups"),
    _cnn("pabp_nets4_n70", 96, 96, 5, 192, nets=4, n=70, potts=(80, 8), form="fused k_experts<6, NG 2>, 4 whole parts, PABP pin refused by n_nets"),
    # ---- n_nets in {1, 4} at the UBE4B shape. With the two-plane split the single-launch kernel needs 70208 bytes of LDS here, two
    # workgroups fit a CU (2 x 70208 <= 163840) and cnn_single_launch keeps the shape: k_cnn<7, 5> (seven row tiles, 100 of 112 rows
    # live). The chunk kernels' UBE4B pin (launch_cnn shape == 1: T 100, CP 128, F 208, chosen by shape alone, no look at n_nets) is
    # reached through PPDE_CNN_CHUNKED=1 only: test_abi_limits_gpu runs these two cases once more in a process with that set.
    _cnn("ube4b_nets1", 104, 104, 5, 208, nets=1, form="k_cnn<7, 5>, 2 parts (1 network cut in two); chunked by knob: pinned backward k_cnn_bwd_chunk<5, 1, true>, grid y = 1"),
    _cnn("ube4b_nets4", 104, 104, 5, 208, nets=4, form="k_cnn<7, 5>, 4 whole parts; chunked by knob: pinned backward, grid y = 4"),
    # ---- kernel sizes, single launch (L = 40: 3 row tiles; K != 5 -> KT = 8 padded tap tables, k_cnn<3, CNN_MAX_K>) ---------------
    _cnn("K1_single", 40, 40, 1, 80, form="k_cnn<3, 8 taps>, 4 parts; T = 40: every row's K-mer is one letter (many exact ties)"),
    _cnn("K2_single", 40, 40, 2, 80, form="k_cnn<3, 8 taps>, 4 parts"),
    _cnn("K4_single", 40, 40, 4, 80, form="k_cnn<3, 8 taps>, 4 parts"),
    _cnn("K6_single", 40, 40, 6, 80, form="k_cnn<3, 8 taps>, 4 parts"),
    _cnn("K8_single", 40, 40, 8, 80, form="k_cnn<3, 8 taps>, 4 parts; all 8 taps live, T = 33"),
    # ---- kernel sizes, chunked (L = 150: rows(T) > 128; CP = 160 > 128 -> the 512-thread chunk kernels, CNN_MAX_K tables) --------
    _cnn("K1_chunked", 150, 150, 1, 300, form="chunked wide <CNN_MAX_K, .., 512>, T = 150: 3 forward chunks, backward windows of 57 outputs"),
    _cnn("K8_chunked", 150, 150, 8, 300, form="chunked wide <CNN_MAX_K, .., 512>, T = 143: 3 forward chunks"),
    # ---- one output row: K = L, T = 1 (a 16-row tile with one live row) -------------------------------------------------------------
    _cnn("T1_L5", 5, 8, 5, 16, form="k_cnn<1, 5>, 3 parts (FP = 16 < 32: no cut), T = 1 at the shortest legal sequence"),
    _cnn("T1_L8", 8, 8, 8, 16, form="k_cnn<1, 8 taps>, 3 parts, T = 1"),
    # ---- width decoupled from length (L = 40, K = 5 unless noted) -------------------------------------------------------------------
    _cnn("C1_F1", 40, 1, 5, 1, form="k_cnn<3, 5>, 3 parts; CP = 32 and FP = 16 are all padding but one column"),
    _cnn("C31_F31", 40, 31, 5, 31, form="k_cnn<3, 5>, 4 parts: FP = 32 is AT the split threshold, 31 live columns"),
    _cnn("C33_F17", 40, 33, 5, 17, form="k_cnn<3, 5>, 4 parts: CP = 64 (one channel in the second k step), FP = 32 with 17 live"),
    _cnn("C33_F33", 40, 33, 5, 33, form="k_cnn<3, 5>, 4 parts: FP = 48, an odd number of 16-column strips for the two halves"),
    _cnn("C130_F512", 40, 130, 5, 512, form="k_cnn<3, 5>, 4 parts: CP = 160, FP = 512 is the last single-launch width"),
    _cnn("C130_F513", 40, 130, 5, 513, form="chunked by FP = 528 > 512 alone: ONE forward chunk (T = 36), wide 512-thread chunk kernels"),
    _cnn("C64_F1000", 40, 64, 5, 1000, form="chunked by FP = 1008: one forward chunk, 256-thread chunk kernels <5, 0, 4, true>"),
    _cnn("C32_F3200", 40, 32, 5, 3200, form="chunked by FP; the backward window's route bitmap (64 rows x 3200 bits = 25600 bytes) exactly fills the "
         "routed gradient's storage (max(256 CP, 64 * 100 * 4) bytes): the widest F a narrow five-tap network may have (F = 3201 .. is refused)"),
    _cnn("L24_C300", 24, 300, 5, 48, form="k_cnn<2, 5>, 4 parts: CP = 320 with 20 rows (channels >> rows)"),
    _cnn("L140_C20", 140, 20, 5, 40, form="chunked by rows alone (T = 136 > 128), narrow: CP = 32, 3 forward chunks, 256 threads"),
    _cnn("K7_wide_chunked", 150, 140, 7, 64, form="chunked (T = 144), CP = 160 > 128 and KT = 8: k_cnn_fwd_chunk / k_cnn_bwd_chunk<CNN_MAX_K, .., 512>"),
    # ---- long sequences (C = 32, F = 64, K = 5, n = 3): the chunk kernels beyond the 4 forward chunks they have ever run -------
    _cnn("L308", 308, 32, 5, 64, n=3, form="chunked, 5 forward / 6 backward chunks; first length past the chain kernels' limit"),
    _cnn("L512", 512, 32, 5, 64, n=3, form="chunked, 8 forward / 9 backward chunks"),
    _cnn("L1000", 1000, 32, 5, 64, n=3, form="chunked, 16 forward / 17 backward chunks"),
    _cnn("L4096", 4096, 32, 5, 64, n=3, form="chunked, 64 forward / 69 backward chunks: the model's declared maximum"),
    # ---- the reference's shape at the last accepted width: CP = 544: cnn_bf_bwd_chunk_lds = 256 * 544 + 8 * 544 + 12 * 1088 + 512
    # = 157184 <= 163840 bytes; CP = 576 (L = 545 .. 576, FP = 1104): 165824 > 163840 -> refused (test_abi_limits_gpu, refusals) ------
    _cnn("ref_L544", 544, 544, 5, 1088, n=2, form="chunked wide, 9 forward / 10 backward chunks, 157184 of 163840 bytes of LDS"),
]

# Seeds found by a CPU search so that case_is_tie_free holds (test_abi_limits_cpu checks it): seed -> weights, wild type, rows.
CNN_SEEDS = {"K7_wide_chunked": 1, "C32_F3200": 3, "pabp_nets2": 1, "ube4b_nets4": 4, "C1_F1": 6, "pabp_nets1_n70": 1, "pabp_nets2_n70": 6,
             "pabp_nets4_n70": 7, "ref_L544": 73}

# The Potts kernel beyond what has run: the general ring kernel with 8 chunk groups per wave serves NC = 17 .. 32 chunks of 16
# residues (launch_potts: g4 false -> potts_energy_grad_kernel<NG, true, 8>), run at Lp = 260 only so far; windows deep inside long
# sequences (the state row's shift and length, set_geom); the whole of a 512-residue sequence.
POTTS_CASES = [dict(name=f"ring_Lp{Lp}_n{n}", L=Lp + 8, Lp=Lp, i0=4, n=n) for Lp in (272, 400, 512) for n in (3, 70)] + [
    dict(name="window_at_930_of_1000", L=1000, Lp=64, i0=930, n=5),         # resident slab, NC = 4, 1000-residue state rows
    dict(name="window_at_4080_of_4096", L=4096, Lp=16, i0=4080, n=5),       # the last 16 residues of the longest sequence
    dict(name="whole_L512", L=512, Lp=512, i0=0, n=5),                      # window = sequence at the window's maximum
]


# Seeds of the rows (as CNN_SEEDS). dH is a difference of two sums of 2 Lp terms whose absolute sum reaches the hundreds while dH
# stays O(1), so at the long windows the fp32 ORACLE's own rounding is of the size of the project's 5e-6: over rows drawn with seeds
# 0 .. 11 its worst row lay between 0.3 and 2.4 of that tolerance at Lp = 400 and 512, and the figure moves with the number of
# threads torch's matmul sums on. The tolerance stays the project's: potts_case_reference evaluates the oracle on ONE thread (so
# err32 is the same number everywhere) and the rows are those on which the oracle then stays below half the tolerance on every
# chain (0.27 .. 0.49 here; test_abi_limits_cpu checks <= 1).
POTTS_SEEDS = {"ring_Lp272_n3": 3, "ring_Lp272_n70": 2, "ring_Lp400_n3": 1, "ring_Lp400_n70": 4, "ring_Lp512_n3": 6, "ring_Lp512_n70": 9,
               "whole_L512": 5}


@functools.lru_cache(maxsize=1)
def potts_512():
    """The Lp = 512 couplings (about 420 MB of fp32), built once per process; shorter windows take J[:Lp, :Lp], h[:Lp]."""
    return synthetic.make_potts(512, seed=77, symmetric=False)


def is_reference_shape(c):
    return c["C"] == c["L"] and c["F"] == 2 * c["L"] and c["K"] == 5 and c["L"] <= 307


@functools.lru_cache(maxsize=4)
def _build_cnn_case(name, seed):
    c = next(k for k in CNN_CASES if k["name"] == name)
    rng = np.random.default_rng(1_000_003 * seed + sum(map(ord, name)))
    wt = rng.integers(0, A, c["L"]).astype(np.uint8)
    states = [make_cnn(c["C"], c["K"], c["F"], 100 * seed + s + 7 * c["C"] + c["F"]) for s in range(c["nets"])]
    idx = make_rows(wt, c["n"], rng, forced=chunk_edge_residues(c["L"], c["K"]) if c["L"] >= 308 else ())
    out = dict(c, wt=wt, states=states, idx=idx, lam=0.0, which=2, J=None, h=None, i0=0)
    if c["potts"]:
        Lp, i0 = c["potts"]
        J, h = synthetic.make_potts(Lp, seed=11 + seed, symmetric=False)
        out.update(J=J, h=h, i0=i0, lam=3.0, which=3)
    return out


def build_cnn_case(name, seed=None):
    """The case's inputs: wt [L], idx [n, L], states (list of state dicts), which / lam and, where given, the Potts window."""
    return _build_cnn_case(name, CNN_SEEDS.get(name, 0) if seed is None else seed)


@functools.lru_cache(maxsize=2)
def build_potts_case(name):
    c = next(k for k in POTTS_CASES if k["name"] == name)
    J, h = potts_512()
    Lp = c["Lp"]
    rng = np.random.default_rng(500 + Lp + c["n"] + c["i0"] + 10_000 * POTTS_SEEDS.get(name, 0))
    wt = rng.integers(0, A, c["L"]).astype(np.uint8)
    return dict(c, wt=wt, idx=make_rows(wt, c["n"], rng, span=(c["i0"], c["i0"] + Lp)), J=J[:Lp, :Lp], h=h[:Lp])


# ---------------------------------------------------------------------------------------------------------------------
# references, err32 and budgets (CPU only; the GPU module recomputes them: they are cheap)
# ---------------------------------------------------------------------------------------------------------------------
def project_tolerances(e, fit, g, lam, which):
    """per-chain energy / fitness tolerances and the gradient's, from the fp64 values"""
    tf = 5e-6 * np.maximum(1.0, np.abs(fit))
    if which == 2:                                   # e = fit, grad = d fit / d x (lamda plays no part)
        return tf, tf, 2e-6 * max(1.0, float(np.abs(g).max()))
    te = 5e-6 * np.maximum(1.0, np.abs(e)) + 4e-6 * lam * np.maximum(1.0, np.abs(fit))
    return te, tf, 2e-6 * max(1.0, lam) * max(1.0, float(np.abs(g).max()))


@functools.lru_cache(maxsize=4)
def cnn_case_reference(name):
    """fp64 reference, fp32 oracle, err32 and budgets of a CNN case: dict with e / fit / g (fp64), e32 / fit32 / g32 (oracle),
    err32 (per quantity: largest over the chains), tol (project) and budget (what the device is held to), branch (quantities
    whose budget is the 4 x err32 one)."""
    import torch
    from helpers import oracle_energy
    import ppde_oracle as orc
    c = build_cnn_case(name)
    fit, g = cnn_fp64(c["states"], c["idx"])
    ix = torch.as_tensor(c["idx"].astype(np.int64))
    if c["which"] == 3:
        dH, gp = potts_fp64(c["J"], c["h"], c["i0"], c["wt"], c["idx"])
        e, g = dH + c["lam"] * fit, gp + c["lam"] * g
        e32, f32, g32 = oracle_energy(c["J"], c["h"], c["i0"], c["wt"], c["states"], c["lam"]).energy_grad(ix)
    else:
        e = fit
        f32, g32 = orc.CnnOracle(c["states"]).fit_grad(ix)
        e32 = f32
    return _with_budgets(dict(e=e, fit=fit, g=g, e32=e32.numpy().astype(np.float64), fit32=f32.numpy().astype(np.float64),
                              g32=g32.numpy().astype(np.float64)), c["lam"], c["which"], is_reference_shape(c))


@functools.lru_cache(maxsize=2)
def potts_case_reference(name):
    import torch
    import ppde_oracle as orc
    c = build_potts_case(name)
    e, g, Hwt = potts_fp64(c["J"], c["h"], c["i0"], c["wt"], c["idx"], with_H=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                         # one summation order on every machine (POTTS_SEEDS)
    try:
        P = orc.PottsOracle(c["J"], c["h"], c["i0"], torch.as_tensor(c["wt"].astype(np.int64)))
        e32, g32 = P.energy_grad(torch.as_tensor(c["idx"].astype(np.int64)))
    finally:
        torch.set_num_threads(threads)
    r = _with_budgets(dict(e=e, fit=np.zeros_like(e), g=g, e32=e32.numpy().astype(np.float64), fit32=np.zeros_like(e),
                           g32=g32.numpy().astype(np.float64)), 0.0, 1, False)
    # H(wt) itself (ppde_model_get_wt_hamiltonian) is another quantity than dH: its own reference, oracle value and err32
    r["H_wt32"] = float(P.wt_H)
    te = 5e-6 * max(1.0, abs(Hwt))
    r["tol"]["H_wt"], r["err32"]["H_wt"] = te, abs(r["H_wt32"] - Hwt)
    r["budget"]["H_wt"] = max(te, 4.0 * r["err32"]["H_wt"])
    if 4.0 * r["err32"]["H_wt"] > te:
        r["branch"].append("H_wt")
    r["H_wt"] = Hwt
    return r


def _with_budgets(r, lam, which, reference_shape):
    te, tf, tg = project_tolerances(r["e"], r["fit"], r["g"], lam, which)
    r["tol"] = dict(e=te, fit=tf, grad=tg)
    r["err32"] = dict(e=float(np.abs(r["e32"] - r["e"]).max()), fit=float(np.abs(r["fit32"] - r["fit"]).max()),
                      grad=float(np.abs(r["g32"] - r["g"]).max()))
    r["budget"], r["branch"] = {}, []
    for k, t in r["tol"].items():
        wide = 4.0 * r["err32"][k]
        if reference_shape or wide <= float(np.min(t)):
            r["budget"][k] = t
        else:
            r["budget"][k] = np.maximum(t, wide)                     # (per chain: 4 x err32 is the budget of at least one)
            r["branch"].append(k)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# chains at ppde_pas_length = 64: paths of up to 127 moves through the one-wave path walk, on the toy fixture's geometry
# ---------------------------------------------------------------------------------------------------------------------
PAS64 = dict(n=16, T=3, pas=64, nmut=0, lam=5.0, seed=64)
PAS64_GAP_TOL = 1e-5                      # relative gap of the exponential race below which a draw counts as a near-tie


def pas64_acc_tol(U):
    """|log_acc - log u| below which an accept bit is a near-tie, for a path of U moves: the project's 2e-4 at paths of up to 5
    moves (test_masked_entry_winning_the_race...) scaled by U / 5 (log_acc sums 2 U log-probabilities)."""
    return 2e-4 * np.asarray(U, dtype=np.float64) / 5.0


def pas64_model():
    """(wt, J, h, i0, Lp, cnn states) of the toy fixture's geometry (L = 24, window 4 .. 19, three reference-shaped networks)"""
    from ppde_amd.encoding import seqs_to_idx
    _, seq, (i0, Lp) = synthetic.PROTEINS["TOY24"]
    wt = seqs_to_idx([seq])[0]
    J, h = synthetic.make_potts(Lp, seed=7)
    return wt, J, h, i0, Lp, [synthetic.make_cnn_state(len(seq), s) for s in range(3)]


def pas64_oracle_run(noise):
    """the oracle's run of the PAS64 chains on `noise` (list of (U, q, u) per iteration), traces and proposal rows kept"""
    import ppde_oracle as orc
    from helpers import oracle_energy
    wt, J, h, i0, Lp, cnn = pas64_model()
    p = PAS64
    en = oracle_energy(J, h, i0, wt, cnn, p["lam"])
    return orc.run(en, np.tile(wt.astype(np.int64), (p["n"], 1)), wt, lambda t: noise[t], p["T"], i0, i0 + Lp - 1, p["pas"], p["nmut"],
                   False, trace=True, keep_probs=True)


def compare_pas64(tr, ref, noise):
    """helpers.compare_runs_up_to_near_ties at PAS64's tolerances, the accept margin held per chain to ITS path length.
    Returns (chains on the oracle's trajectory to the end, notes, mask of those chains)."""
    from helpers import compare_runs_up_to_near_ties
    n_same, notes, same = compare_runs_up_to_near_ties(tr, ref, noise, gap_tol=PAS64_GAP_TOL, acc_tol=float(pas64_acc_tol(2 * PAS64["pas"] - 1)))
    for b, t, what, margin in notes:
        if what == "accept":
            assert margin <= pas64_acc_tol(int(noise[t][0][b])), (b, t, margin)
    return n_same, notes, same


def trace_of(ref, T, mu_max):
    """an oracle run in the layout of Chains.trace(): flat [T, 2 pas - 1, n] (-1 beyond U), accepted, log_acc, U"""
    n = ref["accepted"].shape[1]
    flat = -np.ones((T, mu_max, n), np.int32)
    for t in range(T):
        f = ref["traces"][t]["flat"].numpy()
        flat[t, :f.shape[0]] = f
    return dict(flat=flat, accepted=ref["accepted"].numpy().astype(np.uint8),
                log_acc=np.stack([ref["traces"][t]["log_acc"].numpy() for t in range(T)]))

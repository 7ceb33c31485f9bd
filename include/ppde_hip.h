/*
 * ppde_hip.h — C ABI of the MI355X (gfx950) PPDE sampler hot path.
 *
 * The reference (pemami4911/ppde) has no FFI: its boundary for this path is the duck-typed Python API
 *   ppde/base_sampler.py:8-15            BaseSampler.run(...)
 *   ppde/protein_samplers/ppde.py:24-192 PPDE_PAS.run(...)
 *   ppde/energy.py:97-140                ProteinProductOfExperts.get_energy / get_energy_and_grads / ...
 * This header is what a ctypes/cffi binding of that API calls (ppde_amd/_hip.py is that binding; the stub a
 * maintainer of the reference would add is shown in INTEGRATION.md). Each entry point names the reference
 * code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success and a negative ppde_status otherwise; ppde_last_error() returns a
 *     thread-local human-readable message for the last failure; nothing throws across the ABI;
 *   - "host" pointers are ordinary host memory owned by the caller; "dev" pointers are device memory on the
 *     model's device (e.g. torch tensors' data_ptr()); the library owns every device buffer it allocates;
 *   - states are residue indices, one byte per residue (alphabet ACDEFGHIKLMNPQRSTVWY -> 0..19,
 *     ppde/third_party/hsu/data_utils.py:48-70); fp32 one-hot [n, L, 20] exists only at the API edge;
 *   - a ppde_model is immutable after its set_* calls and may be shared by several ppde_chains; a
 *     ppde_chains owns one HIP stream (and every scratch buffer its kernels and captured graphs touch)
 *     and is not thread-safe; the stateless calls (ppde_energy_grad ...) share one scratch set per model
 *     and must not run concurrently with each other on the same model.
 *
 * Shape limits (checked where the shape is given -- ppde_model_create, the set_* call, ppde_chains_create; violations return
 * PPDE_ERR_INVALID with a message and leave the object as it was, nothing falls back; tests/test_abi_limits_{cpu,gpu}.py run
 * each limit at its edge):
 *   - alphabet 20; sequence length 5 <= L <= 4096 for the model, L <= 307 for ppde_chains (a chain's
 *     L*20 proposal logits live in the registers of one 512-thread workgroup);
 *   - Potts window 1 <= Lp <= min(L, 512), anywhere in the sequence (the kernel reads a transposed copy of the window's
 *     letters: no limit on the state row): windows of more than 128 residues stream through an LDS ring of at most 32 chunks
 *     of 16 residues, shorter ones keep a resident slab of <= 32 KiB pieces per wave;
 *   - supervised expert: 1..4 networks of one shape, kernel size 1 <= K <= min(8, L), C >= 1 channels, F >= 1 features, as
 *     independent numbers. Up to 128 output rows (T = L - K + 1), F <= 512 and a shape of which two workgroups fit a CU's
 *     LDS run the single-launch kernel; longer or wider networks take the chunked kernels, which hold 64 rows of ALL channels
 *     (padded to a multiple of 32: CP; features to a multiple of 16: FP) in LDS: 264 CP + 12 FP + 512 <= 163840 bytes. That
 *     bounds the WIDTH, not the length: C <= 608 at small F, C <= 544 at F = 2C. For networks of the reference's shape
 *     (C = L, F = 2L) it means L <= 544; ppde_model_set_cnn refuses a wider one and names the bound in channels. The chunked
 *     kernels also need FP <= 32 * max(CP, 20 * taps) (taps = 5 for K = 5, else 8): F <= 3200 for narrow five-tap networks
 *     (the exact-fp32 build, PPDE_CNN_BF16=0, has its own form of this bound: FP <= 32 * the padded row stride of CP channels);
 *   - transformer expert: head width 24, 32 or 64, dim a multiple of 8 (<= 1536; padded to a multiple of 128 internally), ffn a
 *     multiple of 128, L <= 256;
 *   - ppde_pas_length 1..64; chain_offset + n_chains < 2^32.
 */
#ifndef PPDE_HIP_H
#define PPDE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPDE_ABI_VERSION 1
#define PPDE_ALPHABET 20
/* `which` bit 3, see ppde_energy_grad */
#define PPDE_WHICH_FULL_GRAD 8

typedef enum {
    PPDE_OK = 0,
    PPDE_ERR_INVALID = -1,     /* bad argument / shape / state */
    PPDE_ERR_HIP = -2,         /* a HIP runtime call failed */
    PPDE_ERR_NOT_ONEHOT = -3,  /* an input row is not a one-hot vector */
    PPDE_ERR_NUMERIC = -4      /* a proposal row had no usable mass: every move masked out or forbidden (the reference raises
                                * ValueError there), a non-finite gradient, or -- device RNG only, whose rows take exp(z - mref)
                                * against a fixed reference mref = min(beta * spread / 2, 64) of the launch -- every admissible
                                * logit 86.6 or more below mref (the normaliser falls below 2^-125: a chain at the mutation cap or
                                * a state outside the library whose best admissible move lies ~23 or more below the current
                                * letters once the gradient's spread reaches 128) or a logit more than 88.7 above it (a spread
                                * beyond 2 * (64 + 88)); the reference, which reduces a maximum per row, carries on there.
                                * ppde_model_set_transformer: the wild type's score is not finite on the weights given */
} ppde_status;

typedef struct ppde_model ppde_model;
typedef struct ppde_chains ppde_chains;

int ppde_abi_version(void);
const char* ppde_last_error(void);
/* number of visible HIP devices, or a negative status */
int ppde_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Model = the product of experts' parameters resident on one device.
 * Replaces the constructors ProteinProductOfExperts.__init__ (ppde/energy.py:72-95),
 * PottsModel.__init__ (ppde/nets.py:245-262) and EnsembleProtein.__init__ (ppde/nets.py:417-424).
 * ---------------------------------------------------------------------------------------------- */

/* L = full sequence length; wt_idx host [L] = wild-type residues (energy.py:95 `wt_onehot`). */
int ppde_model_create(ppde_model** out, int device, int L, const uint8_t* wt_idx);
int ppde_model_destroy(ppde_model* m);

/* Potts couplings J host [Lp, Lp, 20, 20] and fields h host [Lp, 20] (potts.pkl `J_ij`, `h_i`,
 * nets.py:247-249); the window covers residues [win_start, win_start + Lp) (nets.py:280).
 * J need not be symmetric: it is symmetrised on upload, M = (J + J^T)/2, which is what autograd of
 * nets.py:287-290 yields (energy.py:108). Also evaluates wt_H (nets.py:262). */
int ppde_model_set_potts(ppde_model* m, const float* J, const float* h, int Lp, int win_start);

/* Supervised CNN ensemble (nets.py:350-376, :412-442): n_nets networks, each
 * conv_w [C, 20, K], conv_b [C], lin_w [F, C], lin_b [F], dec_w [F], dec_b [1] on the host. */
int ppde_model_set_cnn(ppde_model* m, int n_nets, int C, int K, int F,
                       const float* const* conv_w, const float* const* conv_b,
                       const float* const* lin_w, const float* const* lin_b,
                       const float* const* dec_w, const float* const* dec_b);

/* Transformer unsupervised expert (nets.py:172-240 `Transformer`, :302-312 `PottsTransformer`): an ESM-2 encoder
 * evaluated on one-hot input, score = sum x * log_softmax(logits) minus the wild type's (nets.py:219-240), under the
 * reference's autocast (fp16 matmuls, fp32 statistics). The reference takes the model from the third-party
 * `esm_one_hot` package + torch hub; here the caller passes ESM-2's parameters (fp32, host), named as in
 * facebookresearch/esm's ESM2: per-layer arrays have n_layers entries. Written for head widths 24, 32 and 64
 * (esm2_t12_35M: dim 480, 20 heads, ffn 1920; esm2_t30_150M: 640, 20, 2560; esm2_t33_650M: 1280, 20, 5120), ffn a multiple
 * of 128, L <= 256. Also evaluates the wild
 * type's score.
 * Range. Every activation and activation gradient is an fp16 tensor (normal range 6.1e-5 .. 65504, subnormals kept). What that
 * supports, measured by rescaling seeded weights against fp64 (tests/test_transformer_range_{cpu,gpu}.py), in
 * terms one can read off a checkpoint's activations: the residual stream (entries of order 1 at unit scale) times 2^-12 .. 2^12,
 * and no entry of it beyond 65504 (at 2^14 it is lost); q against k (entries of order 0.1 and 1) times 2^-12 .. 2^13 in either
 * direction; v against out_proj times 2^-14 .. 2^13; layer-norm outputs (gains) times 2^-14 .. 2^11 with the matrices behind them
 * scaled back: within these the distance from fp64 stays within twice what it is at unit scale (gradient 9e-4 of its largest row,
 * d embedding 1.6e-3). Logits up to 80 in magnitude and one stream channel 8 times the others are held at 5e-3 and 2.5e-3 of the
 * gradient; attention rows with one dominant key (scores of order 16) at 8e-2 .. 1.3e-1, which is fp16's rounding of such scores
 * and not the kernels': there the gradient has one digit.
 * Refusals, both leaving the expert that was there answering bit for bit (the new one is built completely, the wild type's score
 * included, before the old one is let go): PPDE_ERR_INVALID naming tensor and layer when a parameter is not finite in fp32 or a
 * matrix entry is not finite once rounded to fp16 (|w| >= 65520), before the device is touched; PPDE_ERR_NUMERIC when the wild
 * type's score comes out non-finite (an fp16 activation overflowed on these weights: every energy would be NaN). A chain whose own
 * activations overflow returns a non-finite energy and gradient and leaves the other chains of its batch bit for bit as they are. */
typedef struct {
    const float* embed;                 /* embed_tokens.weight [33][dim] (also the tied LM-head projection) */
    const float* const* q_w; const float* const* q_b;       /* layers.i.self_attn.{q,k,v,out}_proj.{weight [dim][dim], bias} */
    const float* const* k_w; const float* const* k_b;
    const float* const* v_w; const float* const* v_b;
    const float* const* o_w; const float* const* o_b;
    const float* const* ln1_w; const float* const* ln1_b;   /* layers.i.self_attn_layer_norm */
    const float* const* ln2_w; const float* const* ln2_b;   /* layers.i.final_layer_norm */
    const float* const* fc1_w; const float* const* fc1_b;   /* [ffn][dim], [ffn] */
    const float* const* fc2_w; const float* const* fc2_b;   /* [dim][ffn], [dim] */
    const float* final_ln_w; const float* final_ln_b;       /* emb_layer_norm_after */
    const float* head_dense_w; const float* head_dense_b;   /* lm_head.dense */
    const float* head_ln_w; const float* head_ln_b;         /* lm_head.layer_norm */
    const float* head_bias;                                 /* lm_head.bias [33] */
} ppde_tf_weights;
int ppde_model_set_transformer(ppde_model* m, int n_layers, int dim, int heads, int ffn, const ppde_tf_weights* w);
/* local score of the wild type (nets.py:188 `wt_score`) for inspection. */
int ppde_model_get_transformer_wt_score(ppde_model* m, float* out_host);

/* Timing hook for bench.py: average duration (microseconds) of the transformer's GEMM kernel, C[M,N] = A[M,K] B[N,K]^T,
 * fp16 operands filled with pseudo-random values, `reps` launches between one HIP event pair. epilogue: 0 bias,
 * 2 bias + residual, 3 bias + GELU (the fc1 form), 4 GELU' (backward through fc2), 5 plain. M, N multiples of 128,
 * K of 64. */
int ppde_transformer_time_gemm(int device, int M, int N, int K, int reps, int epilogue, float* avg_us);

/* Diagnostics for the parity tests: an fp16 activation of the last stateless evaluation that used the transformer
 * expert, converted to fp32. what: 0 layer input, 1 q|k|v, 2 (not kept: the backward rebuilds the attention probabilities), 3 post-attention stream,
 * 4 GELU' of the fc1 pre-activation (what the forward keeps for the backward; all of `layer`), 5 final stream, 6 logits, 7 d logits, 8 d embedding, 9 d tokens,
 * 10 / 11 attention output / d q|k|v of the layer evaluated last. The workspace holds ONE chunk of chains (PPDE_TF_WORK_GB; after an
 * evaluation in several chunks: the last one): `count` beyond the buffer's padded rows x width is PPDE_ERR_INVALID. */
int ppde_debug_transformer_read(ppde_model* m, int what, int layer, float* out_host, int64_t count);

/* The fc1 GEMM timed IN SITU for bench.py's roofline object: one stateless transformer evaluation (energy + gradient)
 * of idx_dev [n, L] with a HIP event pair around every fc1 launch (real activations, real neighbouring kernels); mean
 * event-to-event time in microseconds and the number of launches timed (= layers). */
int ppde_transformer_time_fc1_in_situ(ppde_model* m, const uint8_t* idx_dev, int n, float* avg_us, int* launches);

/* lamda of e = dH + lamda * fit (energy.py:74, :99-100). */
int ppde_model_set_lamda(ppde_model* m, float lamda);

/* wt_H (nets.py:262) for inspection. */
int ppde_model_get_wt_hamiltonian(ppde_model* m, float* out_host);

/* ------------------------------------------------------------------------------------------------
 * Stateless evaluations at the API edge (device pointers; `stream` is a hipStream_t or NULL).
 * ---------------------------------------------------------------------------------------------- */

/* fp32 one-hot x_dev [n, L, 20] -> idx_dev [n, L]. Fails with PPDE_ERR_NOT_ONEHOT (after a stream sync)
 * if some row is not exactly one 1.0 and nineteen 0.0. */
int ppde_onehot_to_idx(ppde_model* m, const float* x_dev, int n, uint8_t* idx_dev, void* stream);
/* idx_dev [n, L] -> fp32 one-hot x_dev [n, L, 20]. */
int ppde_idx_to_onehot(ppde_model* m, const uint8_t* idx_dev, int n, float* x_dev, void* stream);

/* get_energy / get_energy_and_grads (energy.py:97-132): e_dev [n], fit_dev [n], and, when grad_dev
 * is not NULL, grad_dev [n, L, 20] = d e.sum() / d x. which: bit 0 = Potts expert, bit 1 = supervised expert,
 * bit 2 = transformer expert; 3 = Potts product of experts, 6 = transformer product of experts
 * (`--unsupervised_expert transformer`), 7 = `potts+transformer`. With which == 2, e = fit and grad = d fit/dx
 * (ProteinSupervised, energy.py:153-160); without bit 1, fit = 0.
 * The gradient follows the reference branch by branch: for the Potts product of experts (3) it is
 * d(dH + lamda * fit)/dx (energy.py:105-108); with the transformer expert (6, 7) the reference computes fit from x
 * but differentiates with respect to the minibatch SLICE of x (energy.py:115, :125), so lamda * d fit/dx never
 * reaches grad_x: grad = d(unsupervised experts)/dx only, while e still holds + lamda * fit (and no CNN backward
 * runs). Bit 3 (PPDE_WHICH_FULL_GRAD, `args.ppde_full_grad`) opts into d e/dx with the supervised term for 6 / 7. */
int ppde_energy_grad(ppde_model* m, const uint8_t* idx_dev, int n, int which,
                     float* e_dev, float* fit_dev, float* grad_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Chains = the sampler state of n independent Markov chains (PPDE_PAS.run, ppde.py:24-192).
 * ---------------------------------------------------------------------------------------------- */

typedef struct {
    int32_t n_chains;        /* chains held by this object (this rank's shard) */
    int32_t max_steps;       /* capacity of the histories (T); run may stop earlier */
    int32_t pas_length;      /* args.ppde_pas_length (ppde.py:12): U ~ randint[1, 2*pas) */
    int32_t nmut_threshold;  /* args.nmut_threshold; 0 = unlimited (ppde.py:15-17) */
    int32_t paper_results;   /* args.paper_results (ppde.py:14,76,148) */
    int32_t min_pos;         /* proposals restricted to residues [min_pos, max_pos] (ppde.py:60-63) */
    int32_t max_pos;
    int32_t which;           /* experts in the energy (+ PPDE_WHICH_FULL_GRAD), as in ppde_energy_grad */
    int32_t rng_mode;        /* 0 = noise supplied by the caller per step (parity with a host generator),
                                1 = counter-based Philox4x32-10 on the device */
    int32_t reuse_grad;      /* 1 = keep energy/gradient of the current state from the previous iteration
                                instead of re-evaluating it (identical results, half the expert calls) */
    int32_t record_after_reset; /* 1 = histories of STATES hold the post-reset state (the reference's
                                --device cpu aliasing artefact); 0 = pre-reset (its cuda behaviour) */
    int32_t trace;           /* 1 = keep per-iteration draws / accept bits / log-acceptance for tests */
    int32_t random_chain;    /* local index of the chain whose trajectory is kept (ppde.py:37,47,142), or -1 */
    int32_t use_graph;       /* 1 = replay iterations from hipGraphs captured at ppde_chains_init (rng_mode 1 only) */
    int32_t n_streams;       /* >1: the chains are cut into this many sub-populations whose iterations run on
                                separate HIP streams and overlap on the GPU (chains are independent, results
                                are unchanged); 0/1 = one stream. rng_mode 1 only. */
    uint64_t seed;           /* Philox key */
    uint64_t chain_offset;   /* global index of local chain 0: results do not depend on the sharding */
} ppde_chain_config;

int ppde_chains_create(ppde_chains** out, ppde_model* m, const ppde_chain_config* cfg);
int ppde_chains_destroy(ppde_chains* c);

/* Design library: allowed_host [L], one word per residue of the full sequence; bit k set = letter k (alphabet
 * ACDEFGHIKLMNPQRSTVWY) may be PROPOSED at that residue, word 0 = the residue is frozen. Enforced exactly inside the
 * forward path of every iteration (ppde.py:98-110), next to the position range (ppde.py:60-63) and the mutation cap:
 *   z[l,k] = -inf where forbidden; p = clamp(softmax(z), 2^-23, 1 - 2^-23) (ppde/utils.py:106-111); p[l,k] = 0 where
 *   forbidden, before any sum of p is formed; p_hat = p / sum(p); draw; log-probability = log clamp(p_hat[win]).
 * So a forbidden entry can never be drawn, while entries masked only by the range or the cap keep the reference's
 * 2^-23 floor (the range alone is no hard limit: about 1.2e-7 per masked entry and draw). The reverse path takes no
 * masks, as the reference treats its own two; Philox counters and the variates consumed do not change; a library of
 * all twenty letters everywhere gives the bits of no library. It constrains moves only: initial states need not lie
 * inside it. "No admissible move" (nothing unmasked and allowed) is flagged PPDE_ERR_NUMERIC as without a library.
 * Valid between ppde_chains_create and ppde_chains_init (the graphs captured there hold the pointer): afterwards
 * PPDE_ERR_INVALID. NULL clears the library. PPDE_ERR_INVALID with a message when a bit >= 20 is set, when an open
 * residue lacks its wild-type letter (the mutation cap's revert move must stay admissible), or when no residue of
 * [min_pos, max_pos] is open. The words are copied; the chains own the device copy. */
int ppde_chains_set_library(ppde_chains* c, const uint32_t* allowed_host /* [L] or NULL */);

/* Reversible mode (off by default). The reference scores the reverse move of sub-step s at the index the FORWARD move chose
 * (ppde.py:122-153, :128-132): in the reverse state that index is the letter the residue already holds, its logit is exactly
 * 0, the move that actually undoes the step is never scored, and the reverse rows take no masks while the forward rows do --
 * so the chains' stationary law is not exp(energy)/Z. With `on` != 0 the accept phase replaces ppde.py:122-153 by a
 * Metropolis-Hastings step of the same forward proposal:
 *   row(g, state) = the forward row: logits (g[l,k] - g[l,state_l]) / 2, the range mask and the mutation-cap mask OF THAT
 *     STATE as -inf, the design library as in ppde_chains_set_library (forbidden: -inf, exactly 0 behind the clamp);
 *   forward path: unchanged (same rows, Philox counters, variates consumed, recorded forward log-probabilities);
 *   reverse row of sub-step s = row(g_y, x_{s+1}), read at the move that undoes the sub-step: (l_s, old_s), old_s the
 *     letter residue l_s held in x_s; logp_rev = log clamp(p_hat[l_s, old_s]);
 *   log_acc = (e_y - e_x) + sum_s (logp_rev_s - logp_fwd_s), accepted when exp(log_acc) >= u, as before;
 *   a path with a reverse move the library forbids (probability exactly 0) is rejected, whatever u is;
 *   the mutation cap is a constraint, not a reset: a proposal with dist(y) >= nmut_threshold is rejected and nothing is
 *     ever reset to the wild type (stationary law exp(E) * 1[dist < threshold] / Z). A rejected proposal records accept
 *     bit 0 and the current energy.
 * The clamp to [2^-23, 1 - 2^-23] makes the log-probabilities of the ratio differ from the draw probabilities at entries on
 * the floor or the ceiling; with a library that folds the range in (no masked-but-drawable entry) the law is exp(energy)/Z
 * over the library up to that. Valid between ppde_chains_create and ppde_chains_init (the captured graphs hold the kernel
 * choice): afterwards PPDE_ERR_INVALID. `on` with paper_results is PPDE_ERR_INVALID: its reject-to-initial-state move is no
 * Metropolis step. Initial states need not lie inside the library: a residue holding a letter outside it never moves (its
 * reverse move is forbidden). */
int ppde_chains_set_reversible(ppde_chains* c, int on);

/* Parallel tempering (off by default; needs reversible mode, where the law at an inverse temperature beta is defined:
 * exp(beta E)/Z_beta over the library). beta_host [n_rungs] is a ladder beta[0] > beta[1] > ... > beta[R-1] > 0, R = n_rungs.
 *   ensembles: R chains with consecutive GLOBAL indices g = chain_offset + local index; chain g belongs to ensemble g / R and
 *     starts on rung g % R;
 *   a chain on rung r runs the reversible iteration above on the energy beta_r * E: every row, forward and reverse, is
 *     row(beta g, state) with logits beta * ((g[l,k] - g[l,state_l]) * 0.5f) in this order of operations (beta = 1 gives the
 *     untempered bits, a power of two commutes with the rounding); masks, library, clamp and zeroing as before;
 *     log_acc = beta * (e_y - e_x) + sum_s (logp_rev_s - logp_fwd_s), accepted when exp(log_acc) >= u; the explicit rejections
 *     and the mutation cap as a constraint are unchanged. Philox counters and the variates consumed do not change;
 *   histories, best states, peek and collect hold the UNTEMPERED energy and fitness; "best" is the largest E on any rung;
 *   swap events: after the accept phase of iteration `it` (0-based) when swap_every > 0 and (it + 1) % swap_every == 0;
 *     event s = (it + 1) / swap_every - 1 pairs, in every ensemble, the rungs (r, r + 1) with r = s (mod 2), r + 1 < R;
 *   swap rule: a = the chain on rung r, b = the chain on rung r + 1, d = (beta_r - beta_{r+1}) * (E_b - E_a) in fp32 on the
 *     post-accept energies, accepted when expf(d) >= u, u the uniform of Philox word .x at counter (global index of the
 *     ensemble's first chain, it, 0x40000000, r), a stream the chain kernels never use. A swap exchanges TEMPERATURES (beta,
 *     rung, and the ensemble's rung -> chain map), never states, gradients, records or histories;
 *   every joint kernel (the product of the rungs' kernels, then the swap) keeps prod_r exp(beta_r E(x_r)) / Z_r invariant;
 *   results do not depend on the sharding (Philox is keyed by global indices). swap_every = 0: a ladder without exchange.
 * A tempering run enqueues propose, experts, accept, swap per iteration: the fused accept + propose launch is not used (the
 * next proposal must see the post-swap beta, the swap the post-accept energy). Valid between ppde_chains_create and
 * ppde_chains_init; n_rungs = 0 or NULL clears it. PPDE_ERR_INVALID with a message, the object unchanged: after init;
 * reversible mode not on; n_rungs > 64; a beta that is not finite and positive, or a ladder not strictly decreasing;
 * swap_every < 0; n_chains or chain_offset no multiple of n_rungs; n_streams > 1. While it is set,
 * ppde_chains_set_reversible(c, 0) is PPDE_ERR_INVALID. The ladder is copied; the chains own the device arrays. */
int ppde_chains_set_tempering(ppde_chains* c, int n_rungs, const float* beta_host, int swap_every);

/* Where the temperatures are now: rung host int32 [n], beta host fp32 [n] (per chain), swap_attempts / swap_accepts host
 * int64 [n / R][R - 1] per (ensemble, pair of rungs r, r + 1). Any pointer may be NULL. Synchronises. PPDE_ERR_INVALID
 * without tempering. */
int ppde_chains_tempering_state(ppde_chains* c, int32_t* rung, float* beta, int64_t* swap_attempts, int64_t* swap_accepts);

/* rung_history host uint8 [steps_done + 1, n]: the rung each chain held after every iteration (row 0: the start). */
int ppde_chains_tempering_history(ppde_chains* c, uint8_t* rung_history);

/* Population annealing (off by default; needs reversible mode, as tempering does, and excludes it): all chains of a DEME share one
 * inverse temperature, which climbs a schedule, and at every step of the schedule the deme is resampled with weights
 * exp(dbeta E) (Hukushima & Iba; Machta): a sequential Monte Carlo sampler with a defined target, exp(beta[s] E)/Z, at every stage.
 *   demes: D chains with consecutive GLOBAL indices g = chain_offset + local index; chain g belongs to deme g / D;
 *   schedule: beta[0] <= beta[1] <= ... <= beta[S], S = n_stages, every entry finite and positive, equal neighbours allowed;
 *   run: every chain starts at beta[0] and runs the reversible iteration of tempering on beta * E, by the same kernels: the same
 *     Philox counters and variates are consumed. Histories, best states, peek and collect hold the UNTEMPERED energy and fitness;
 *   events: behind the accept phase of iteration `it` (0-based) when (it + 1) % every == 0 and s = (it + 1) / every - 1 < S.
 *     Stage s resamples every deme and then moves every chain from beta[s] to beta[s + 1]. Past the schedule nothing happens and
 *     beta stays at beta[S]. events_cap = min(S, max_steps / every);
 *   plan of one deme at an event, in fp64 on the fp32 inputs: e_i = the post-accept energy of the deme's chain i (history row
 *     it + 1); dbeta = (double)beta[s + 1] - (double)beta[s]; a non-finite e_i has weight 0; E_max = the largest finite energy;
 *     w_i = exp(dbeta ((double)e_i - E_max)); C_i = the inclusive prefix sum in index order, W = C_{D-1}; u = the uniform of
 *     Philox word .x at counter (global index of the deme's first chain, it, 0x40000001, 0), a stream nothing else draws from;
 *     tau_j = (j + u) (W / D), j = 0..D-1; ancestor a_j = #{i : C_i <= tau_j}, clamped to the last i with w_i > 0; n_i = the
 *     number of j with a_j = i (systematic resampling: n_i is floor or ceil of D w_i / W). A deme without a finite energy keeps
 *     the identity and records log_mean_w = -inf, ess = 0;
 *   slot rule: a chain with n_i >= 1 keeps its slot, parent[i] = i. The dead slots (n_i = 0), in increasing order, receive the
 *     surplus list in order: every i in increasing order, repeated n_i - 1 times. Copies therefore read only rows nobody writes;
 *     a survivor's slot, archive and best state go on undisturbed;
 *   a replaced slot d takes from p = parent[d] everything the next iteration and the observers read for a chain: the state (and
 *     its transposed copy for the Potts kernel), the energy, fitness and mutation count it continues from, its gradient row under
 *     gradient reuse, row it + 1 of both histories, and row it + 1 of the random trajectory when d is the recorded chain. Row
 *     it + 1 thereby describes the population AFTER selection, which is what ppde_chains_peek returns. The running best of slot d
 *     follows the accept phase's strict rule: if the copied energy exceeds best_e, then best_e, best_f, best_t = it + 1 and
 *     best_state follow it. The last accept bit and the traces stay the slot's own Metropolis result;
 *   recorded per event, [events_cap] rows: parent int32 [n] (LOCAL index of the ancestor; the identity where nothing was
 *     replaced); pre_energy fp32 [n], the energies the plan saw (the history row is rewritten: this is the only place they
 *     survive, and what a pilot run's next schedule is designed from); log_mean_w fp64 [n / D] = log(W / D) + dbeta E_max, whose
 *     sum over the events is the deme's estimate of log(Z_{beta[S]} / Z_{beta[0]}); ess fp64 [n / D] = W^2 / sum w_i^2;
 *   observers: recorder, pair counts, archive and move statistics are defined by what ppde_chains_peek returns; their kernels run
 *     behind the selection and hold unchanged -- except that the statistics' moved <= accepts no longer follows: a replaced
 *     slot jumps without accepting;
 *   a schedule of equal betas all 1 gives, bit for bit, the histories, states, bests and traces of the reversible run; results do
 *     not depend on the sharding.
 * An annealing run enqueues propose, experts, accept and two selection kernels (ppde_amd/csrc/anneal.h) per iteration, unfused,
 * valid under graph replay and eager issue alike; on an iteration without an event both return at once. A run without annealing
 * enqueues nothing new and makes no additional runtime call. Valid between ppde_chains_create and ppde_chains_init; NULL clears it.
 * PPDE_ERR_INVALID with a message, the object unchanged: after init; reversible mode not on; tempering set; deme outside 2..1024;
 * n_chains or chain_offset no multiple of deme; every < 1; n_stages outside 1..4096; events_cap == 0; a beta that is not finite
 * and positive, or a decreasing pair; n_streams > 1. While it is set, ppde_chains_set_tempering and ppde_chains_set_reversible(c, 0)
 * are PPDE_ERR_INVALID. The schedule is copied; the chains own the device arrays; a failed allocation is PPDE_ERR_HIP and leaves
 * nothing half-set. */
typedef struct {
    int32_t deme;        /* D, 2..1024 */
    int32_t every;       /* >= 1 */
    int32_t n_stages;    /* S, 1..4096 */
    const float* beta;   /* [S + 1] */
} ppde_anneal_config;
int ppde_chains_set_annealing(ppde_chains* c, const ppde_anneal_config* cfg /* NULL clears */);
/* Deme size, event capacity and the events that have happened (follows ppde_chains_steps_done). Any pointer may be NULL.
 * PPDE_ERR_INVALID without annealing. */
int ppde_chains_annealing_shape(ppde_chains* c, int32_t* deme, int32_t* events_cap, int32_t* events_done);
/* Events [first_event, first_event + n_events) to the host, and the inverse temperature each chain holds now. Synchronises; any
 * pointer may be NULL. PPDE_ERR_INVALID without annealing, before init, or for events beyond events_done. */
int ppde_chains_annealing_read(ppde_chains* c, int first_event, int n_events,
                               int32_t* parent /* [n_events][n] */, float* pre_energy /* [n_events][n] */,
                               double* log_mean_w /* [n_events][n / D] */, double* ess /* [n_events][n / D] */,
                               float* beta_now /* [n] */);

/* Adaptive population annealing: the same mode (the same demes, events, plan, slot rule, copies, records and observers as above),
 * except that no schedule is given: at every event each deme chooses its own next beta, the largest step whose incremental weights
 * still leave an effective sample size of ess_target times the deme (Jasra et al. 2011; Zhou, Johansen & Aston 2016). All
 * arithmetic is fp64 on the fp32 inputs, on the device, inside the captured iteration graph:
 *   run: every chain starts at beta_start; iteration `it` is event s = (it + 1) / every - 1 when (it + 1) % every == 0 and
 *     s < events_cap = min(max_stages, max_steps / every). Past events_cap nothing happens and each deme keeps the beta it has;
 *   step of one deme at an event: beta_cur = beta[first chain of the deme], b0 = (double)beta_cur; e_i the post-accept energies
 *     (history row it + 1), F the number of finite ones, E_max the largest finite one, x_i = (double)e_i - E_max.
 *     F == 0: beta stays (and the plan's no-finite-energy rule applies: identity, log_mean_w = -inf, ess = 0).
 *     dmax = (double)beta_end - b0 <= 0: the deme has arrived, beta_next = beta_cur, and the event runs the plan with dbeta = 0, as
 *     equal neighbours of a fixed schedule do. Otherwise, with ESS(d) = (sum w_i)^2 / sum w_i^2, w_i = exp(d x_i) over the finite
 *     e_i (ESS(0) = F, non-increasing in d >= 0) and target = (double)ess_target F:
 *       if ESS(dmax) >= target: d = dmax; otherwise lo = 0, hi = dmax and 48 times mid = 0.5 (lo + hi), ESS(mid) >= target ?
 *       lo = mid : hi = mid; then d = max(lo, (double)min_step);
 *     beta_next = beta_end if d >= dmax or (float)(b0 + d) >= beta_end, otherwise (float)(b0 + d), rounded to nearest;
 *   the event then runs the plan above unchanged with dbeta = (double)beta_next - b0 -- weights, systematic resampling on the
 *     same Philox stream, slot rule, parent, pre_energy, log_mean_w, ess -- and sets beta = beta_next for the deme's chains;
 *   recorded in addition, per event and deme: beta_before = beta_cur and beta_after = beta_next.
 * What follows: deme by deme the adaptive run IS the fixed-schedule run on that deme's recorded beta path (beta_start,
 * beta_after[0], beta_after[1], ...), bit for bit; its estimate of log(Z_end / Z_start) is the sum of the same log_mean_w, but
 * with steps that depend on the states that estimate is consistent in D and no longer unbiased, and only demes that have arrived
 * at beta_end estimate the same ratio. ESS >= 1 always, so with ess_target <= 1 / D the first event jumps to beta_end (D = 2 with
 * ess_target = 0.5 always jumps). min_step bounds the number of stages by (beta_end - beta_start) / min_step and is what moves a
 * deme whose ESS falls below the target at any d > 0.
 * The adaptive form and ppde_chains_set_annealing are one mode: a successful call of either replaces what either set, NULL to
 * either clears it, ppde_chains_annealing_shape and ppde_chains_annealing_read serve both, and while either is set the other
 * setters refuse as described above. PPDE_ERR_INVALID with a message, the object unchanged: every refusal of
 * ppde_chains_set_annealing that concerns the object, deme and every (after init; reversible mode not on; tempering or
 * recombination set; deme outside 2..1024; n_chains or chain_offset no multiple of deme; every < 1; events_cap == 0;
 * n_streams > 1); max_stages outside 1..4096; beta_start or beta_end not finite and positive; beta_start >= beta_end; ess_target
 * not finite or outside (0, 1); min_step not finite or < beta_end * 2^-20 (so that every step changes beta in fp32). A failed
 * allocation is PPDE_ERR_HIP and leaves nothing half-set. */
typedef struct {
    int32_t deme;        /* D, 2..1024 */
    int32_t every;       /* >= 1 */
    int32_t max_stages;  /* 1..4096 */
    float beta_start;    /* finite, > 0, < beta_end */
    float beta_end;
    float ess_target;    /* rho, inside (0, 1) */
    float min_step;      /* >= beta_end * 2^-20 */
} ppde_anneal_adaptive_config;
int ppde_chains_set_annealing_adaptive(ppde_chains* c, const ppde_anneal_adaptive_config* cfg /* NULL clears */);
/* The inverse temperature every deme held before and after events [first_event, first_event + n_events). Under a fixed schedule
 * these are beta[s] and beta[s + 1] for every deme. Synchronises; either pointer may be NULL. PPDE_ERR_INVALID without annealing,
 * before init, or for events beyond events_done. */
int ppde_chains_annealing_read_betas(ppde_chains* c, int first_event, int n_events,
                                     float* beta_before /* [n_events][n / D] */, float* beta_after /* [n_events][n / D] */);

/* Recombination (off by default; needs reversible mode): every `every`-th iteration the chains of a deme are paired and each
 * pair proposes to exchange a segment of open residues -- a Metropolis move on the pair with a symmetric proposal, which keeps
 * the product law prod_i exp(E(x_i)) / Z of the reversible chains invariant (the crossover of evolutionary Monte Carlo, Liang &
 * Wong 2000; DNA shuffling in the laboratory). It excludes tempering, annealing, paper_results and n_streams > 1.
 *   demes: D chains with consecutive GLOBAL indices g = chain_offset + local index; D even, D >= 2;
 *   open list: the residues l of [min_pos, max_pos] in increasing order -- with a design library only those whose word is not 0;
 *     S_o = their number. Only these are ever exchanged; frozen residues stay with their chain;
 *   events: iteration `it` (0-based) is event s = (it + 1) / every - 1 when (it + 1) % every == 0; events_cap = max_steps / every.
 *     The event runs behind the accept phase of that iteration and in front of the observers;
 *   pairing (round robin, circle method): m = D - 1, r = s mod m; slot m of the deme pairs with slot r, slot i < m, i != r with
 *     (2r - i) mod m. A perfect matching; every two slots meet once in m consecutive events. The lower slot of a pair is a, the
 *     other b;
 *   draw, one per pair: Philox4x32-10 at counter (global index of a, it, 0x40000002, 0) -- a stream nothing else draws from, in
 *     both rng_modes -- gives x, y, z, w; i1 = mulhi32(x, S_o), i2 = mulhi32(y, S_o), lo = min, hi = max, u = the 24-bit uniform
 *     of z; the segment = the open residues open[lo..hi];
 *   children: a' = a with b's letters at the segment's residues, b' = b with a's. The same draw on (a', b') gives (a, b) back.
 *     differ = the segment residues at which a and b differ; child_dist = each child's mutation count against the wild type;
 *   evaluation: both children's whole rows go to the proposal slot and the run's expert evaluation of that slot follows (the same
 *     `which`); E', f' = the proposal slot's energy and fitness;
 *   decision, in fp32 and in this order, E_a, E_b = the post-accept energies (history row it + 1): d = (E'_a - E_a) + (E'_b - E_b);
 *     outcome 3: an E' is not finite (rejected); 2: a mutation cap is set and a child_dist >= nmut_threshold (rejected, never through
 *     u); 4: forbidden patterns are set and a child is not free (rejected, never through u; ppde_chains_set_forbidden_patterns);
 *     1: expf(d) >= u (accepted); 0: rejected by u. A pair with differ = 0 takes the same path (d = 0: accepted);
 *   on acceptance each of the two slots takes from its child everything the next iteration and the observers read for a chain: the
 *     state (and its transposed copy), the energy, fitness and mutation count it continues from, its gradient row under gradient
 *     reuse, row it + 1 of both histories and of the random trajectory for the recorded chain, the running best by the accept
 *     phase's strict rule. The last accept bit and the traces stay the slot's own Metropolis result. Row it + 1 and
 *     ppde_chains_peek describe the population AFTER the event;
 *   recorded per event, [events_cap] rows of [n]: partner int32 (LOCAL index), lo, hi int32 (indices into the open list), differ,
 *     child_dist int32, outcome uint8, log_ratio fp32 (d, the same in both slots of a pair), pre_energy, child_energy fp32;
 *   results do not depend on the sharding.
 * The host decides which iterations are events: only there are three more launches enqueued (ppde_amd/csrc/recombine.h: the
 * children, the experts on the proposal slot, the decision), behind a plain accept kernel; nothing fuses across an event. Captured
 * graph segments have lengths that are multiples of `every` (every * floor(100 / every) and `every` itself up to 100, `every` up
 * to 1000, none beyond; PPDE_GRAPH_LEN only when it is such a multiple) and are replayed only from positions that are multiples of
 * `every`; ppde_chains_run issues iterations eagerly up to the next such position. A run without the mode enqueues nothing new and
 * makes no additional runtime call. Valid between ppde_chains_create and ppde_chains_init, and after ppde_chains_set_library;
 * NULL clears it. PPDE_ERR_INVALID with a message, the object unchanged: after init; reversible mode not on; tempering or
 * annealing set; deme odd or < 2; n_chains or chain_offset no multiple of deme; every < 1; events_cap == 0; n_streams > 1. While it
 * is set, ppde_chains_set_library, ppde_chains_set_tempering, ppde_chains_set_annealing and ppde_chains_set_reversible(c, 0) are
 * PPDE_ERR_INVALID. A failed allocation is PPDE_ERR_HIP and leaves nothing half-set. */
typedef struct {
    int32_t deme;        /* D, even, >= 2 */
    int32_t every;       /* >= 1 */
} ppde_recombine_config;
int ppde_chains_set_recombination(ppde_chains* c, const ppde_recombine_config* cfg /* NULL clears */);
/* Deme size, the open list, event capacity and the events that have happened (follows ppde_chains_steps_done). Synchronises; any
 * pointer may be NULL. PPDE_ERR_INVALID without the mode or before init. */
int ppde_chains_recombination_shape(ppde_chains* c, int32_t* deme, int32_t* n_open, int32_t* open_sites /* [n_open] or NULL */,
                                    int32_t* events_cap, int32_t* events_done);
/* Events [first_event, first_event + n_events) to the host, [n_events][n] each. Synchronises; any pointer may be NULL.
 * PPDE_ERR_INVALID without the mode, before init, or for events beyond events_done. */
int ppde_chains_recombination_read(ppde_chains* c, int first_event, int n_events,
                                   int32_t* partner, int32_t* lo, int32_t* hi, int32_t* differ, int32_t* child_dist,
                                   uint8_t* outcome, float* log_ratio, float* pre_energy, float* child_energy);

/* Forbidden sequence patterns (off by default; needs reversible mode): "never produce this short pattern anywhere" as one more
 * indicator in the target. The reversible chains' stationary law becomes exp(beta E(x)) 1[dist(x) < thr] 1[x free] / Z (beta under
 * tempering or annealing). The proof is the mutation cap's: a Metropolis step that explicitly rejects every proposal outside a
 * set, from a state inside it, is reversible with respect to the law restricted to that set.
 *   patterns: M of them, 1 <= M <= 32; pattern m is length[m] elements, 1 <= length[m] <= 8, element j = element[m][j], a non-empty
 *     set of letters as a 20-bit word (bit k = letter k of ACDEFGHIKLMNPQRSTVWY, the design library's convention). A state x
 *     matches pattern m at start p when 0 <= p <= L - length[m] and x[p + j] is in element j for every j. Windows run over the
 *     WHOLE sequence [0, L): frozen residues and residues outside [min_pos, max_pos] are context;
 *   native sites: allow_native != 0 exempts every (m, p) at which the WILD TYPE matches, whatever the chain puts there later;
 *     allow_native = 0 exempts nothing. active[p] bit m = pattern m is checked at start p: p + length[m] <= L and (m, p) not exempt.
 *     x is FREE when no active (m, p) matches;
 *   accept phase: a proposal y that is not free is rejected explicitly, next to the cap's dist(y) < thr, never through the test
 *     against u. It records what a cap rejection records: accept bit 0, the current energy in row it + 1; the trace's log_acc stays
 *     the computed value. The forward path, the Philox counters and the variates consumed do not change. Only y is checked, not
 *     the intermediate states of its path;
 *   initial states: every one must be free: ppde_chains_init with one that is not is PPDE_ERR_INVALID and names the chain, the
 *     pattern and the position. With allow_native = 0 and a wild type that matches, the setter succeeds and leaves a note that
 *     names the pattern and the position in ppde_last_error (the run is legal from other free states);
 *   recombination: a pair with a child that is not free is rejected with outcome 4, checked after the non-finite energy (3) and
 *     the cap (2) and before u. A run without patterns never writes 4;
 *   tempering's swap and annealing's selection move free states only and do not change. Both rng_modes, every `which` and
 *     n_streams > 1 work (one veto launch per sub-population on its stream);
 *   vetoes int64 [n][M]: vetoes[b][m] = the iteration proposals of chain b that were not free and whose lowest matching active
 *     pattern was m, counted whether or not the proposal would otherwise have been accepted. Recombination's children are not
 *     counted (their record is outcome 4). ppde_chains_init zeroes them.
 * One more kernel per iteration (ppde_amd/csrc/motif.h: k_motif_veto, one wave per chain, on the proposal slot behind its expert
 * evaluation and in front of the accept or fused launch) and one inside a recombination event (between the children and their
 * evaluation). A run without the mode enqueues nothing new and computes the bits it computed before. Valid between
 * ppde_chains_create and ppde_chains_init, before or after ppde_chains_set_library; NULL clears it. PPDE_ERR_INVALID with a message,
 * the object unchanged: after init; reversible mode not on (hence with paper_results); n_patterns outside 1..32; a length outside
 * 1..8 or above L; an element inside its pattern's length that is 0 or has a bit >= 20 set; no active (m, p) at all. While it is
 * set, ppde_chains_set_reversible(c, 0) is PPDE_ERR_INVALID. A failed allocation is PPDE_ERR_HIP and leaves nothing half-set. */
typedef struct {
    int32_t n_patterns;         /* M, 1..32 */
    const int32_t* length;      /* [M] 1..8 */
    const uint32_t* element;    /* [M][8]; words behind a pattern's length are ignored */
    int32_t allow_native;
} ppde_motif_config;
int ppde_chains_set_forbidden_patterns(ppde_chains* c, const ppde_motif_config* cfg /* NULL clears */);
/* M, allow_native and the active words. Any pointer may be NULL. PPDE_ERR_INVALID without the mode. */
int ppde_chains_forbidden_shape(ppde_chains* c, int32_t* n_patterns, int32_t* allow_native, uint32_t* active /* [L] */);
/* The counters so far. Synchronises. PPDE_ERR_INVALID without the mode or before init. */
int ppde_chains_forbidden_read(ppde_chains* c, int64_t* vetoes /* [n][M] */);
/* The scan on its own (stateless): the same device function over n rows of residue indices [n][L] on the device, against the
 * model's wild type. first_pattern[i] = the lowest active pattern row i matches and first_pos[i] its lowest start position; -1 / -1
 * for a free row. Synchronises the stream. The config is checked as by the setter. */
int ppde_motif_scan(ppde_model* m, const ppde_motif_config* cfg, const uint8_t* idx_dev, int n, int32_t* first_pattern_dev,
                    int32_t* first_pos_dev, void* stream);

/* Recorder (off by default): thinned samples of the population and per-site letter counts, written on the device inside the
 * iteration loop (one more kernel behind the accept phase -- behind the swap, with tempering -- of every iteration of a recording
 * run; no host round trip; valid under graph replay and eager issue alike). A run without a recorder enqueues nothing new.
 *   recorded iterations: the state after t completed iterations when t > burn_in and (t - burn_in) % every == 0, into row
 *     (t - burn_in) / every - 1; rows_cap = (max_steps - burn_in) / every; rows_done follows ppde_chains_steps_done;
 *   slots: rung = -1: every chain is a slot (slot = local chain index); rung = r >= 0 (tempering only): one slot per ensemble,
 *     filled by the chain that holds rung r AFTER that iteration's swap (the chain whose rung_history entry in row t is r);
 *   a row holds, per slot, exactly what ppde_chains_peek returns after that iteration: idx from the current states (post-reset
 *     in the default mode), energy / fitness = row t of the histories (untempered), chain = the local index of the chain;
 *   site_counts[l][k] = number of recorded (row, slot) pairs with letter k at residue l, over all recorded rows, kept whether or
 *     not samples are (keep_samples = 0: counts only, no per-row buffers). ppde_chains_init zeroes them.
 * The recorder changes no other result: histories, best states, traces and Philox streams are those of the run without it.
 * Valid between ppde_chains_create and ppde_chains_init (the graphs hold the pointers), after ppde_chains_set_tempering when
 * rung >= 0; NULL clears it. PPDE_ERR_INVALID with a message, the object unchanged: after init; every < 1; burn_in < 0; no row
 * would fit (rows_cap == 0); rung < -1; rung >= 0 without tempering or rung >= n_rungs; keep_samples not 0 or 1; n_streams > 1
 * (the counters have one owner per launch). While a recorder with rung >= 0 is set, ppde_chains_set_tempering (to clear or to
 * replace) is PPDE_ERR_INVALID. The buffers ([rows_cap][slots] rows of state bytes, energy, fitness, chain) belong to the
 * chains; a failed allocation is PPDE_ERR_HIP and leaves no recorder half-set. */
typedef struct {
    int32_t burn_in;      /* >= 0 */
    int32_t every;        /* >= 1 */
    int32_t rung;         /* -1: every chain is a slot; r >= 0 (tempering only): one slot per ensemble = the chain holding rung r */
    int32_t keep_samples; /* 1: keep states/energy/fitness/chain per row; 0: site counts only */
} ppde_record_config;
int ppde_chains_set_recorder(ppde_chains* c, const ppde_record_config* cfg /* NULL clears */);
/* rows recorded so far, row capacity, slots per row. Any pointer may be NULL. PPDE_ERR_INVALID without a recorder. */
int ppde_chains_recorder_shape(ppde_chains* c, int32_t* rows_done, int32_t* rows_cap, int32_t* slots);
/* Rows [first_row, first_row + n_rows) to the host; site_counts covers ALL rows recorded so far. Synchronises; any pointer may
 * be NULL. PPDE_ERR_INVALID: rows beyond rows_done; a sample pointer when keep_samples = 0. */
int ppde_chains_recorder_read(ppde_chains* c, int first_row, int n_rows,
                              uint8_t* idx /* [n_rows][slots][L] */, float* energy, float* fitness /* [n_rows][slots] */,
                              int32_t* chain /* [n_rows][slots], local chain index */, uint64_t* site_counts /* [L][20] */);

/* Pair counts (off by default): the second moment next to the recorder's first, counted on the device by one more kernel directly
 * behind the recorder's in every iteration (ppde_amd/csrc/pairs.h); a run without them enqueues nothing new.
 *   pair_counts[i][a][j][b] = number of recorded (row, slot) pairs with letter a at residue sites[i] and letter b at residue
 *     sites[j]: the same recorded iterations and slots as site_counts (the recorder's burn_in, every and rung), read from the
 *     current states, so kept whether or not samples are. As a matrix [S 20][S 20] it is the Gram matrix of the one-hot rows of
 *     the recorded samples restricted to `sites`: symmetric, diagonal blocks diag(site_counts[sites[i]]). ppde_chains_init zeroes it.
 *   sites: S strictly increasing residues of the full sequence, 0-based; n_sites = 0 with sites = NULL selects every residue.
 *     The list is copied.
 * Valid with a recorder set and before ppde_chains_init (the graphs hold the pointers); NULL clears them. PPDE_ERR_INVALID with a
 * message, the object unchanged: no recorder; after init; n_sites < 0 or > L; n_sites > 0 with sites = NULL; n_sites = 0 with a
 * list; a site outside [0, L); sites not strictly increasing. While pair counts are set, ppde_chains_set_recorder (to clear or to
 * replace) is PPDE_ERR_INVALID: clear the pair counts first. The chains own the buffers; a failed allocation is PPDE_ERR_HIP and
 * leaves nothing half-set. */
typedef struct {
    int32_t n_sites;       /* 0 (with sites = NULL): every residue */
    const int32_t* sites;  /* [n_sites], strictly increasing, each in [0, L) */
} ppde_pair_config;
int ppde_chains_set_pair_counts(ppde_chains* c, const ppde_pair_config* cfg /* NULL clears */);
/* Number of sites and the list itself. Any pointer may be NULL. PPDE_ERR_INVALID without pair counts. */
int ppde_chains_pair_counts_shape(ppde_chains* c, int32_t* n_sites, int32_t* sites /* [S] or NULL */);
/* The counts over ALL rows recorded so far, full and symmetric. Synchronises. PPDE_ERR_INVALID without pair counts or before init. */
int ppde_chains_pair_counts_read(ppde_chains* c, uint64_t* pair_counts /* [S][20][S][20] */);

/* Archive (off by default): each chain's K best DISTINCT sequences, each with its own energy, kept on the device in n K L bytes
 * whatever the run length, by one more kernel (ppde_amd/csrc/archive.h) behind the accept phase -- behind the swap, with tempering,
 * and behind the recorder's kernels -- of every iteration of an archiving run: no host round trip, valid under graph replay and
 * eager issue alike. A run without an archive enqueues nothing new and makes no additional runtime call.
 *   candidate: chain b after t completed iterations offers what ppde_chains_peek would return: the letters of its current state
 *     with row t of the two histories (untempered, as everywhere). ppde_chains_init offers t = 0, every iteration `it` of every
 *     ppde_chains_run offers t = it + 1.
 *   skipped, decided before anything else: a chain whose mutation count is 0 (what peek returns as dist): the wild type is never
 *     archived; and an energy that is not finite. In the default mode a mutation-cap reset leaves the wild type in the current
 *     state while row t still holds the energy of the state that was reset away: that pair is skipped, never mislabelled, and the
 *     state that triggered the reset is not archived either -- the archive holds only states the chain continued from. In the
 *     default mode with a cap every entry therefore has 1 <= dist < nmut_threshold, and best_idx (ppde_chains_collect) may hold
 *     a state AT the cap that the archive lacks.
 *   online rule, in this order: 1. an archived entry of this chain has the same L letters: nothing happens, the entry keeps its
 *     first energy and step; 2. else count < K: inserted with step = t; 3. else m = the entry of lowest energy, among entries of
 *     equal energy the one with the latest step: replaced when e > energy[m] (strict, like the running best), else nothing.
 *     An entry that was evicted and is visited again re-enters under rule 2 / 3 with its later step.
 * The archive changes no other result: histories, best states, traces, recorder rows and Philox streams are those of the run
 * without it. It holds in the default, library, reversible and tempering modes (the chains of every rung are archived), for every
 * `which`, both gradient policies and both rng_modes. It is independent of the recorder and the pair counts.
 * Valid between ppde_chains_create and ppde_chains_init (the graphs hold the pointers); NULL clears it. PPDE_ERR_INVALID with a
 * message, the object unchanged: after init; k outside 1..32; paper_results (after a rejection its history row holds the energy of
 * the state that was left while the chain continues from its initial state: a mismatched pair with no flag to see it by);
 * n_streams > 1. The chains own the buffers; a failed allocation is PPDE_ERR_HIP and leaves nothing half-set. ppde_chains_init
 * empties the archive (a second init too). */
typedef struct {
    int32_t k;   /* entries per chain, 1..32 */
} ppde_archive_config;
int ppde_chains_set_archive(ppde_chains* c, const ppde_archive_config* cfg /* NULL clears */);
/* Entries per chain. The pointer may be NULL. PPDE_ERR_INVALID without an archive. */
int ppde_chains_archive_shape(ppde_chains* c, int32_t* k);
/* Every chain's entries sorted by (energy descending, step ascending; steps are unique within a chain); slots beyond count[b] hold
 * idx 255, energy -inf, fitness 0, step -1. Synchronises; any pointer may be NULL. PPDE_ERR_INVALID without an archive or before
 * init. */
int ppde_chains_archive_read(ppde_chains* c, uint8_t* idx /* [n][K][L] */, float* energy, float* fitness /* [n][K] */,
                             int32_t* step /* [n][K] */, int32_t* count /* [n] */);

/* Move statistics (off by default): how often the chains accept, how far an accepted path carries them, how acceptance falls with
 * the path length, which residues ever change -- counted on the device by one more small kernel (ppde_amd/csrc/stats.h) behind the
 * accept phase of every iteration of such a run, last behind the swap, the recorder's kernels and the archive's: no host round trip,
 * valid under graph replay and eager issue alike. A run without statistics enqueues nothing new and makes no additional runtime call.
 *   notation: n chains, R' = max(n_rungs, 1), M = mu_max = 2 pas_length - 1; for iteration `it` (0-based), t = it + 1.
 *   x_t[b], d_t[b]: the letters and `dist` ppde_chains_peek returns for chain b after t completed iterations (after a mutation-cap
 *     reset; under paper_results after the fall-back to the initial state). A_it[b]: the accept bit of iteration it, what peek's
 *     `accepted` shows after it and what a trace run's accepted[it][b] holds (an explicit rejection of reversible mode is 0).
 *     U_it[b]: the path length the iteration used, as a trace run's U[it][b], after the clamp min(max(U, 1), min(mu_max, max_u)).
 *     r = r_it[b]: the rung chain b held while it ran iteration it = rung_history[it][b] (row it: before that iteration's swap);
 *     0 without tempering. h = number of residues l with x_{t-1}[b][l] != x_t[b][l].
 *   counters, all int64, zeroed by ppde_chains_init (a second init too), cumulative over every ppde_chains_run since; iteration it adds
 *     iters        [n][R']  1                          accepts      [n][R']  A_it[b]
 *     moved        [n][R']  h > 0                      jump_sum     [n][R']  h
 *     dist_sum     [n][R']  d_t[b]                     wt_returns   [n][R']  d_{t-1}[b] > 0 && d_t[b] == 0
 *     len_attempts [R'][M]  1 at [r][U_it[b] - 1]      len_accepts  [R'][M]  A_it[b] at [r][U_it[b] - 1]
 *     site_changes [R'][L]  1 at [r][l] for every changed residue l of chain b (only with per_site = 1)
 *   so sum_r iters[b][r] = steps_done; sum_b iters[.][r] = sum_u len_attempts[r][u] (accepts alike); sum_l site_changes[r][l] =
 *   sum_b jump_sum[b][r]; and without paper_results moved <= accepts elementwise (an accepted path may undo itself: h may be 0, and
 *   h <= U) -- except in an annealing run, where a slot replaced by the selection jumps (h up to L) without accepting. Everything is an integer: the results do not depend on any summation order.
 * The statistics change no other result: histories, best states, traces, recorder rows, pair counts, archive and Philox streams are
 * those of the run without them. They hold in the default, library, reversible and tempering modes and with paper_results, for every
 * `which`, both gradient policies and both rng_modes. They are independent of recorder, pair counts and archive.
 * Valid between ppde_chains_create and ppde_chains_init (the graphs hold the pointers), and after ppde_chains_set_tempering when
 * there is a ladder (R' is fixed at the set call); NULL clears them. PPDE_ERR_INVALID with a message, the object unchanged: after
 * init; per_site not 0 or 1; n_streams > 1. While statistics are set, ppde_chains_set_tempering (to clear or to replace) is
 * PPDE_ERR_INVALID. The chains own the buffers; a failed allocation is PPDE_ERR_HIP and leaves nothing half-set. */
typedef struct {
    int32_t per_site;   /* 1: keep site_changes; 0: not */
} ppde_stats_config;
int ppde_chains_set_stats(ppde_chains* c, const ppde_stats_config* cfg /* NULL clears */);
/* R', M and per_site. Any pointer may be NULL. PPDE_ERR_INVALID without statistics. */
int ppde_chains_stats_shape(ppde_chains* c, int32_t* n_rungs /* R' */, int32_t* n_lengths /* M */, int32_t* per_site);
/* The counters so far. Synchronises; any pointer may be NULL. PPDE_ERR_INVALID without statistics, before init, or with
 * site_changes when per_site = 0. */
int ppde_chains_stats_read(ppde_chains* c, int64_t* iters, int64_t* accepts, int64_t* moved, int64_t* jump_sum,
                           int64_t* dist_sum, int64_t* wt_returns,            /* [n][R'] each */
                           int64_t* len_attempts, int64_t* len_accepts,        /* [R'][M] */
                           int64_t* site_changes);                             /* [R'][L] */

/* Start from idx0_dev [n, L] (ppde.py:35-47): evaluates the initial energies, fills history row 0. */
int ppde_chains_init(ppde_chains* c, const uint8_t* idx0_dev);

/* Run `steps` iterations of ppde.py:65-153. For rng_mode 0 the caller supplies, for these iterations,
 *   U_dev int32 [steps, n]          path lengths in [1, 2*pas)        (torch.randint, ppde.py:67)
 *   q_dev fp32  [sum_t max_u(t), n, L*20]  Exp(1) variates, max_u(t) = max_b U[t,b]  (multinomial, ppde.py:109)
 *   u_dev fp32  [steps, n]          accept uniforms                  (torch.rand_like, ppde.py:138)
 *   max_u host int32 [steps]
 * and for rng_mode 1 passes NULLs. Asynchronous: returns once the work is enqueued. */
int ppde_chains_run(ppde_chains* c, int steps, const int32_t* U_dev, const float* q_dev,
                    const float* u_dev, const int32_t* max_u);

/* Block until enqueued work is done; reports PPDE_ERR_NUMERIC if a proposal row degenerated (see the code's comment above). */
int ppde_chains_sync(ppde_chains* c);

int ppde_chains_steps_done(ppde_chains* c);

/* Current population (after the mutation-cap reset) and what the reference logs every log_every
 * (ppde.py:155-170): any pointer may be NULL. idx host [n, L], energy/fitness host [n] = last history
 * row, accepted host [n] = last accept bits, dist host [n] = mutation counts. Synchronises. */
int ppde_chains_peek(ppde_chains* c, uint8_t* idx, float* energy, float* fitness, uint8_t* accepted, int32_t* dist);

/* Final collect (ppde.py:172-192): best state per chain by max energy over history (first index on ties),
 * histories [steps_done+1, n], random trajectory [steps_done+1, L]. Any pointer may be NULL. Synchronises. */
int ppde_chains_collect(ppde_chains* c, uint8_t* best_idx, float* best_energy, float* best_fitness,
                        int32_t* best_step, float* energy_history, float* fitness_history, uint8_t* random_traj);

/* hipGraph bookkeeping for bench.py: graphs are captured and instantiated by ppde_chains_init (segments of
 * 100 and 20 iterations when max_steps allows, or PPDE_GRAPH_LEN), never inside ppde_chains_run;
 * captures_in_run counts violations of that (always 0), replayed/eager_steps say how the iterations of all runs
 * so far were issued. Any pointer may be NULL. */
int ppde_chains_graph_stats(ppde_chains* c, int32_t* captures, int32_t* captures_in_run,
                            int64_t* replayed_steps, int64_t* eager_steps);

/* Trace buffers (cfg.trace = 1): flat host int32 [steps_done, 2*pas-1, n] (-1 = not drawn),
 * accepted host uint8 [steps_done, n], log_acc host fp32 [steps_done, n], U host int32 [steps_done, n]. */
int ppde_chains_trace(ppde_chains* c, int32_t* flat, uint8_t* accepted, float* log_acc, int32_t* U);

/* Device RNG inspection (tests): fills q_dev [n, L*20], u_dev [n], U_dev [n] with what iteration `it`,
 * sub-step `s` would use in rng_mode 1. The device RNG draws the categorical of a sub-step in two levels (residue, then
 * letter: the same law as the reference's flat race, ppde.py:106-110, with L + 20 variates instead of L*20): row b of q_dev
 * holds the Exp(1) variates of the residue race in [0, L), those of the letter race in [L, L + 20), and 1.0 beyond. */
int ppde_chains_philox_dump(ppde_chains* c, int it, int s, float* q_dev, float* u_dev, int32_t* U_dev);

/* Timing hooks for bench.py: average duration in microseconds of the Potts energy+gradient kernel over
 * the launches recorded since the last reset, measured with HIP events on the chains' stream. */
int ppde_chains_time_potts_kernel(ppde_chains* c, int reps, float* avg_us);

/* The same for ALL experts of the chains' energy (cfg.which, with gradients), e.g. the fused Potts + CNN launch of the
 * Potts product of experts: `reps` evaluations of the current states into the proposal slot between one HIP event
 * pair on the chains' stream; average microseconds per evaluation. */
int ppde_chains_time_experts(ppde_chains* c, int reps, float* avg_us);

/* The same kernel timed IN SITU: runs `iters` real iterations of a Potts-only energy (which = 1; eagerly, on the chains'
 * stream) with a stop event bound to every kernel's dispatch; avg_us = mean time from the predecessor kernel's end to the
 * Potts launch's end in microseconds, launches = how many were timed, avg_dispatch_us (may be NULL) = mean of the Potts
 * dispatches' own start -> end stamps (0 if the runtime does not report them). The iterations count towards steps_done.
 * rng_mode 1 only. */
int ppde_chains_time_potts_in_situ(ppde_chains* c, int iters, float* avg_us, int* launches, float* avg_dispatch_us);

#ifdef __cplusplus
}
#endif
#endif /* PPDE_HIP_H */

// Population annealing (ppde_chains_set_annealing, include/ppde_hip.h): the selection step of a deme.
//
// k_select_plan and k_select_copy are launched behind k_accept_temp of EVERY iteration `it` of an annealing run, in this order.
// The iteration index is the device counter + the node-local offset, as in k_swap and k_record, so a captured graph segment is
// valid at any offset. There is an event when (it + 1) % every == 0 and s = (it + 1) / every - 1 < S; otherwise both kernels
// return on the first (uniform) branch.
//
// k_select_plan: one 256-thread workgroup per deme of D <= 1024 consecutive chains, four consecutive chains per thread.
//   e_i = post-accept energy (history row it + 1), fp64 from here on: E_max over the finite ones (DPP max, one LDS exchange),
//   w_i = exp(dbeta (e_i - E_max)), 0 for a non-finite e_i; C = inclusive prefix sums in index order (four per thread, a DPP scan
//   of the threads' totals per wave, the waves' totals through LDS), W = C_{D-1};
//   tau_j = (j + u) (W / D), u from Philox at (first chain of the deme, it, 0x40000001, 0) -- a stream nothing else draws from;
//   a_j = #{i : C_i <= tau_j} by binary search over C in LDS, clamped to the last i with w_i > 0; n_i by LDS integer atomics
//   (integers: order-free); the ranks of the dead slots (n_i = 0) and of the surplus list (every i, n_i - 1 times, increasing) by
//   integer prefix sums; the k-th dead slot takes the k-th entry of the surplus list, everyone else is its own parent.
//   Writes row s of parent / pre_energy / log_mean_w / ess, and beta[b] = schedule[s + 1] for its chains (nobody reads beta in
//   this launch).
// k_select_plan_adaptive (ppde_chains_set_annealing_adaptive; both plan kernels are the text of anneal_plan.h, included twice
//   below): the same plan behind a step the deme chooses itself. With
//   b0 = beta[first chain of the deme], x_i = e_i - E_max, F finite energies and ESS(d) = (sum w)^2 / sum w^2, w_i = exp(d x_i), it
//   takes the largest d in (0, beta_end - b0] with ESS(d) >= rho F: the whole remainder if that passes, otherwise 48 bisection steps,
//   and at least min_step. Every ESS is one workgroup reduction: per-wave DPP sums, the waves' partials through LDS (two buffers
//   in turns: one barrier per evaluation), read and added by EVERY thread in the same order, so all threads hold the same bits
//   and the loop branches uniformly. beta_next = (float)(b0 + d), or beta_end once that is reached; the plan then runs on
//   db = (double)beta_next - b0, exactly as k_select_plan runs on the schedule's difference, and records (beta, beta_next) of the
//   event. Static LDS: k_select_plan 16 480 bytes, the adaptive form 16 624 (+ 2 x 8 doubles, + 4 ints).
// k_select_copy: one workgroup per chain, returns unless parent[b] != b. A replaced slot takes from its parent everything the
//   next iteration and the observers read for a chain: the state row and its T4 bytes, ChainRec::cur_e / cur_f / dist_cur, the
//   grad_cur row under gradient reuse, row it + 1 of both histories (and of rtraj for the recorded chain), and moves its running
//   best by the accept phase's strict rule. Parents are survivors, and survivors are never written: no thread reads what another
//   thread of the launch writes (k_swap's rule), which is why the plan and the copy are two launches.
// No global atomics; every global write is a plain store.
#pragma once
#include "common.h"
#include "pas.h"

#define ANNEAL_BLOCK 256
#define ANNEAL_CPT 4                         // chains per thread of the plan
#define ANNEAL_DMAX (ANNEAL_BLOCK * ANNEAL_CPT)
#define ANNEAL_NW (ANNEAL_BLOCK / 64)
#define ANNEAL_STREAM 0x40000001u

struct AnnealArgs {
    const int* it_base;         // device iteration base (graph replay) or NULL
    int it_local;
    int n, D, every, S;         // chains of the object, deme size, iterations per stage, stages
    Geom g;
    int n_pad;
    RngKey key;
    int rec_stride, random_chain, reuse;
    const float* sched;         // [S + 1] the schedule
    float* beta;                // [n]
    unsigned char* rec;         // [n] chain records
    uint8_t* cur;               // [n][Ls]
    uint8_t* curT;              // T4 copy (potts.h)
    float* grad_cur;            // [n][N] (gradient reuse)
    float* e_hist;              // [T+1][n]
    float* f_hist;
    uint8_t* best_state;        // [n][L]
    uint8_t* rtraj;             // [T+1][L]
    int* parent;                // [events_cap][n] local index of the ancestor
    float* pre_energy;          // [events_cap][n]
    double* log_mean_w;         // [events_cap][n / D]
    double* ess;
};

// what k_select_plan_adaptive takes besides (a.sched is not read there)
struct AnnealStepArgs {
    float beta_end, rho, min_step;
    int cap;                    // events_cap
    float* beta_pair;           // [2][events_cap][n / D]: beta before / after every event
};

// stage of the event behind iteration `it`, or -1
__device__ __forceinline__ int anneal_stage(const AnnealArgs& a, int& it) {
    typedef const __attribute__((address_space(4))) int* cptr;
    it = (a.it_base ? *(cptr)(a.it_base) : 0) + a.it_local;
    if ((it + 1) % a.every != 0) return -1;
    const int s = (it + 1) / a.every - 1;
    return s < a.S ? s : -1;
}

// inclusive prefix sum of a double over the 64 lanes: wave_scan_incl_i's steps on both halves of the value
__device__ __forceinline__ double wave_scan_incl_d(double v) {
    v += dpp_d<0x111>(v);                            // row_shr:1 (lanes shifted in from outside the row read 0.0)
    v += dpp_d<0x112>(v);
    v += dpp_d<0x114>(v);
    v += dpp_d<0x118>(v);
    v += dpp_rows_d<DPP_BCAST15, 0xA>(v);
    v += dpp_rows_d<DPP_BCAST31, 0xC>(v);
    return v;
}

// exclusive prefix of per-thread integer totals over the workgroup and their grand total; xw holds ANNEAL_NW ints
__device__ __forceinline__ int anneal_scan_excl_i(int v, int* xw, int& total) {
    const int incl = wave_scan_incl_i(v);
    __syncthreads();                                 // (the previous use of xw is over)
    if ((threadIdx.x & 63) == 63) xw[threadIdx.x >> 6] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < ANNEAL_NW; ++w) {
        const int t = xw[w];
        off += w < (int)(threadIdx.x >> 6) ? t : 0;
        total += t;
    }
    return off + incl - v;
}

// ESS numerator and denominator of the adaptive step at increment d: tot = sum w, sq = sum w^2 over the deme, the same bits in
// every thread (all threads add the waves' partials in the order of the waves). xa: 2 x 2 ANNEAL_NW doubles, used in turns -- a
// thread may write the next evaluation's buffer while others still read this one's, and the barrier in between orders the rest.
__device__ __forceinline__ void anneal_ess_sums(double d, const double (&x)[ANNEAL_CPT], const bool (&fin)[ANNEAL_CPT], double* xa,
                                                int& turn, double& tot, double& sq) {
    double t = 0.0, q = 0.0;
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        const double w = fin[r] ? exp(d * x[r]) : 0.0;
        t += w;
        q += w * w;
    }
    t = wave_sum_d(t);
    q = wave_sum_d(q);
    double* buf = xa + 2 * ANNEAL_NW * (turn & 1);
    if ((threadIdx.x & 63) == 0) { buf[threadIdx.x >> 6] = t; buf[ANNEAL_NW + (threadIdx.x >> 6)] = q; }
    __syncthreads();
    ++turn;
    tot = 0.0; sq = 0.0;
#pragma unroll
    for (int k = 0; k < ANNEAL_NW; ++k) { tot += buf[k]; sq += buf[ANNEAL_NW + k]; }
}

#define ANNEAL_PLAN_ADAPTIVE 0
#include "anneal_plan.h"
#undef ANNEAL_PLAN_ADAPTIVE
#define ANNEAL_PLAN_ADAPTIVE 1
#include "anneal_plan.h"
#undef ANNEAL_PLAN_ADAPTIVE

__global__ __launch_bounds__(ANNEAL_BLOCK) void k_select_copy(AnnealArgs a) {
    int it;
    const int s = anneal_stage(a, it);
    if (s < 0) return;
    const int d = blockIdx.x;
    const int p = a.parent[(size_t)s * a.n + d];
    if (p == d) return;
    const Geom g = a.g;
    const int tid = threadIdx.x;
    if (a.reuse) {
        const float4* src = (const float4*)(a.grad_cur + (size_t)p * g.N);
        float4* dst = (float4*)(a.grad_cur + (size_t)d * g.N);
        for (int k = tid; k < g.N / 4; k += ANNEAL_BLOCK) dst[k] = src[k];
    }
    {
        const uint32_t* src = (const uint32_t*)(a.cur + (size_t)p * g.Ls);
        uint32_t* dst = (uint32_t*)(a.cur + (size_t)d * g.Ls);
        for (int k = tid; k < g.Ls / 4; k += ANNEAL_BLOCK) dst[k] = src[k];
    }
    if (g.Lp > 0)                                    // the padded Potts window's bytes, at store_letter's addresses
        for (int wl = tid; wl < 16 * g.NC; wl += ANNEAL_BLOCK)
            a.curT[state_t4_offset_dev(g.NC, a.n_pad, d, wl)] = a.curT[state_t4_offset_dev(g.NC, a.n_pad, p, wl)];
    if (tid >= 64) return;
    const size_t hrow = (size_t)(it + 1) * a.n;
    const float e = a.e_hist[hrow + p], f = a.f_hist[hrow + p];
    ChainRec* rd = (ChainRec*)(a.rec + (size_t)d * a.rec_stride);
    const ChainRec* rp = (const ChainRec*)(a.rec + (size_t)p * a.rec_stride);
    const bool better = e > rd->best_e;              // strict, like the accept phase
    const bool traj = d == a.random_chain;
    if (better || traj)
        for (int l = tid; l < g.L; l += 64) {
            const uint8_t v = a.cur[(size_t)p * g.Ls + g.sh + l];
            if (better) a.best_state[(size_t)d * g.L + l] = v;
            if (traj) a.rtraj[(size_t)(it + 1) * g.L + l] = v;
        }
    if (tid == 0) {
        const float ce = rp->cur_e, cf = rp->cur_f;
        const int dist = rp->dist_cur;
        a.e_hist[hrow + d] = e;
        a.f_hist[hrow + d] = f;
        rd->cur_e = ce; rd->cur_f = cf; rd->dist_cur = dist;
        if (better) { rd->best_e = e; rd->best_f = f; rd->best_t = it + 1; }
    }
}

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

__global__ __launch_bounds__(ANNEAL_BLOCK) void k_select_plan(AnnealArgs a) {
    int it;
    const int s = anneal_stage(a, it);
    if (s < 0) return;
    __shared__ double C[ANNEAL_DMAX];                // inclusive prefix sums of the weights
    __shared__ int cnt[ANNEAL_DMAX];                 // offspring counts
    __shared__ int lst[ANNEAL_DMAX];                 // the surplus list
    __shared__ double xd[2 * ANNEAL_NW];
    __shared__ float xf[ANNEAL_NW];
    __shared__ int xi[ANNEAL_NW];
    const int D = a.D, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int first = blockIdx.x * D;                // local index of the deme's first chain
    const int i0 = tid * ANNEAL_CPT;
    const float* erow = a.e_hist + (size_t)(it + 1) * a.n + first;
    const double db = (double)a.sched[s + 1] - (double)a.sched[s];

    float e[ANNEAL_CPT];
    bool fin[ANNEAL_CPT];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        const int i = i0 + r;
        e[r] = i < D ? erow[i] : -INFINITY;
        fin[r] = i < D && fabsf(e[r]) < INFINITY;    // (false for NaN and both infinities)
        if (fin[r]) mx = fmaxf(mx, e[r]);
        cnt[i] = 0;
    }
    mx = wave_max(mx);
    if (lane == 0) xf[wave] = mx;
    __syncthreads();
    float emax_f = xf[0];
#pragma unroll
    for (int w = 1; w < ANNEAL_NW; ++w) emax_f = fmaxf(emax_f, xf[w]);
    const bool any = emax_f > -INFINITY;             // a finite energy in the deme
    const double emax = (double)emax_f;

    double w[ANNEAL_CPT], tot = 0.0, sq = 0.0;
    int last = -1;
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        w[r] = fin[r] ? exp(db * ((double)e[r] - emax)) : 0.0;
        tot += w[r];
        sq += w[r] * w[r];
        if (w[r] > 0.0) last = i0 + r;
    }
    const double incl = wave_scan_incl_d(tot);
    const double sq_w = wave_sum_d(sq);
    last = (int)wave_max((float)last);               // (indices below 2^24: exact in fp32)
    if (lane == 63) xd[wave] = incl;
    if (lane == 0) { xd[ANNEAL_NW + wave] = sq_w; xi[wave] = last; }
    __syncthreads();
    double off = 0.0, sumsq = 0.0;
    int last_pos = -1;
#pragma unroll
    for (int k = 0; k < ANNEAL_NW; ++k) {
        off += k < wave ? xd[k] : 0.0;
        sumsq += xd[ANNEAL_NW + k];
        last_pos = max(last_pos, xi[k]);
    }
    {
        double c = off + incl - tot;                 // exclusive prefix of this thread
#pragma unroll
        for (int r = 0; r < ANNEAL_CPT; ++r) { c += w[r]; C[i0 + r] = c; }
    }
    __syncthreads();
    const double W = C[D - 1];
    const bool select = any && W > 0.0;

    if (select) {
        const U4 rnd = philox4x32_10(U4{a.key.chain_lo + (uint32_t)first, (uint32_t)it, ANNEAL_STREAM, 0u}, a.key.k0, a.key.k1);
        const double u = (double)unif_from_bits(rnd.x), step = W / (double)D;
#pragma unroll
        for (int r = 0; r < ANNEAL_CPT; ++r) {
            const int j = i0 + r;
            if (j >= D) continue;
            const double tau = ((double)j + u) * step;
            int lo = 0, hi = D;                      // first i with C_i > tau = #{i : C_i <= tau}
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (C[mid] <= tau) lo = mid + 1; else hi = mid;
            }
            atomicAdd(&cnt[min(lo, last_pos)], 1);
        }
    }
    __syncthreads();
    int nd = 0, ns = 0, c_i[ANNEAL_CPT];
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        c_i[r] = (select && i0 + r < D) ? cnt[i0 + r] : 1;
        nd += c_i[r] == 0 ? 1 : 0;
        ns += c_i[r] > 1 ? c_i[r] - 1 : 0;
    }
    int total_dead, total_surplus;
    int dx = anneal_scan_excl_i(nd, xi, total_dead);
    int sx = anneal_scan_excl_i(ns, xi, total_surplus);
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r)
        for (int k = 1; k < c_i[r]; ++k) lst[min(sx++, ANNEAL_DMAX - 1)] = i0 + r;     // (sum (n_i - 1)+ = dead slots <= D - 1)
    __syncthreads();
    const size_t row = (size_t)s * a.n + first;
    const float b_next = a.sched[s + 1];
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        const int i = i0 + r;
        if (i >= D) continue;
        int p = i;
        if (c_i[r] == 0) { p = lst[min(dx, ANNEAL_DMAX - 1)]; ++dx; }
        a.parent[row + i] = first + p;
        a.pre_energy[row + i] = e[r];
        a.beta[first + i] = b_next;
    }
    if (tid == 0) {
        const size_t cell = (size_t)s * (a.n / D) + blockIdx.x;
        a.log_mean_w[cell] = select ? log(W / (double)D) + db * emax : -INFINITY;
        a.ess[cell] = select ? W * W / sumsq : 0.0;
    }
}

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

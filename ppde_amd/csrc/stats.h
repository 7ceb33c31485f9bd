// Move statistics of a run (ppde_chains_set_stats, include/ppde_hip.h): acceptances, jump distances, mutation counts, wild-type
// returns per (chain, rung), attempts and acceptances per (rung, path length), changes per (rung, residue).
//
// One launch behind the accept phase (behind k_swap, the recorder's kernels and k_archive) of EVERY iteration of a run with
// statistics; the iteration index is the device counter + the node-local offset, as in k_record, so a captured graph segment is
// valid at any offset. Iteration `it` compares what ppde_chains_peek returns after it + 1 completed iterations -- the state rows of
// `cur` (post-reset), ChainRec::dist_cur, ChainRec::acc_last -- with the observer's own copy of the state and mutation count after
// `it` completed iterations: prev [2][n][Ls], two buffers, iteration `it` READS buffer it & 1 and WRITES buffer (it + 1) & 1, so no
// workgroup of a launch reads what another one writes; pdist [n]. ppde_chains_init fills buffer 0 and pdist.
//   rung:        row `it` of rung_hist, the rung the chain held while it ran the iteration (k_swap of this iteration has already
//                written row it + 1 and rung[b]); 0 without a ladder.
//   path length: NOT ChainRec::Ucur -- under gradient reuse the accept of `it` is fused with the propose of it + 1, and the record
//                holds the next path when an observer runs. rng_mode 1: the Philox draw of (chain, it, stream 0) again; rng_mode 0:
//                the iteration's U_in. Both with propose_prefetch's clamp min(max(U, 1), min(mu_max, mu_cap)).
// k_stats has three workgroup roles:
//   sites  (the first site_blocks workgroups, only with per_site): a workgroup owns 16 bytes of the state row, threads are chains,
//          as in k_record; a changed residue byte adds one to the workgroup's LDS cell (rung, byte); the owning thread of each cell
//          then does a plain 64-bit load, add and store on site_changes.
//   chains (the next ceil(n / 4)): one wave per chain, as in k_archive: h = residue bytes that differ between the two rows (XOR,
//          byte compare under arch_dword_mask, wave reduction), then lane 0 owns the chain's six counters at its rung and its
//          pdist, and the wave writes the chain's row of the OTHER prev buffer.
//   lengths (the last workgroup): it owns len_attempts / len_accepts [R][M], gathered over all chains in LDS.
// Every global counter has exactly one owner per launch, there are no global atomics (LDS only), and no thread reads what another
// thread of the launch writes (k_swap's rule). Only integers: the results do not depend on any order. Pad bytes are never counted.
#pragma once
#include "common.h"
#include "pas.h"
#include "archive.h"

#define STAT_BLOCK 256
#define STAT_NW (STAT_BLOCK / 64)
#define STAT_RMAX 64

struct StatArgs {
    const int* it_base;         // device iteration base (graph replay) or NULL
    int it_local;
    int n, R, M, L, Ls, sh;     // chains, max(n_rungs, 1), mu_max, residues, state-row stride, byte of residue 0
    int rng_mode, pas, mu_cap;
    RngKey key;
    int rec_stride;
    const unsigned char* rec;   // [n] chain records (ChainRec::acc_last, ::dist_cur)
    const uint8_t* cur;         // [n][Ls]
    const uint8_t* rung_hist;   // [T+1][n], or NULL (no ladder)
    const int* U_in;            // [n] caller-supplied path lengths of this iteration (rng_mode 0)
    int site_blocks;            // workgroups of the sites role: ceil(Ls / 16) with per_site, else 0
    uint8_t* prev;              // [2][n][Ls] buffer it & 1: the state after `it` completed iterations
    int* pdist;                 // [n]     its mutation count
    long long *iters, *accepts, *moved, *jump_sum, *dist_sum, *wt_returns;   // [n][R]
    long long *len_attempts, *len_accepts;                                    // [R][M]
    long long* site_changes;                                                  // [R][L], or NULL
};

__device__ __forceinline__ int stat_iteration(const StatArgs& a) {
    typedef const __attribute__((address_space(4))) int* cptr;
    return (a.it_base ? *(cptr)(a.it_base) : 0) + a.it_local;
}
__device__ __forceinline__ int stat_rung(const StatArgs& a, int it, int b) {
    return a.rung_hist ? min((int)a.rung_hist[(size_t)it * a.n + b], a.R - 1) : 0;
}

// ppde_chains_init: the mutation counts of the initial population, next to its copy of the state rows
__global__ void k_stats_init(const unsigned char* rec, int rec_stride, int* pdist, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) pdist[b] = ((const ChainRec*)(rec + (size_t)b * rec_stride))->dist_cur;
}

__device__ __forceinline__ void stats_sites_role(const StatArgs& a, int it, const uint8_t* prev, unsigned int* s_cnt) {
    const int wg = blockIdx.x;
    const int nd = a.Ls >> 2;                                                // dwords of a state row
    const int d0 = 4 * wg;                                                   // first dword this workgroup owns
    const int l0 = 16 * wg - a.sh;                                           // residue of its first byte
    const int cells = a.R * 16;
    for (int i = threadIdx.x; i < cells; i += STAT_BLOCK) s_cnt[i] = 0u;
    __syncthreads();
    for (int b = threadIdx.x; b < a.n; b += STAT_BLOCK) {
        const unsigned int* x = (const unsigned int*)(a.cur + (size_t)b * a.Ls) + d0;
        const unsigned int* p = (const unsigned int*)(prev + (size_t)b * a.Ls) + d0;
        unsigned int v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (d0 + j < nd) v[j] = (x[j] ^ p[j]) & arch_dword_mask(d0 + j, a.sh, a.L);
        if ((v[0] | v[1] | v[2] | v[3]) == 0u) continue;                    // (most chains, most iterations)
        const int r = stat_rung(a, it, b);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((v[j >> 2] >> (8 * (j & 3))) & 0xffu) atomicAdd(&s_cnt[r * 16 + j], 1u);   // (LDS)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += STAT_BLOCK) {                  // the owner of (rung, residue)
        const int r = i >> 4, l = l0 + (i & 15);
        const unsigned int s = s_cnt[i];
        if (l < 0 || l >= a.L || s == 0u) continue;
        a.site_changes[(size_t)r * a.L + l] += (long long)s;
    }
}

// dynamic LDS: max(2 * R * M, 16 * R) words (the cells of the last workgroup / of a sites workgroup)
__global__ __launch_bounds__(STAT_BLOCK) void k_stats(StatArgs a) {
    extern __shared__ unsigned int s_len[];
    const int it = stat_iteration(a);
    const size_t buf = (size_t)a.n * a.Ls;
    const uint8_t* prev = a.prev + (size_t)(it & 1) * buf;                   // read by this launch
    uint8_t* next = a.prev + (size_t)((it + 1) & 1) * buf;                   // written by this launch
    if ((int)blockIdx.x < a.site_blocks) {
        stats_sites_role(a, it, prev, s_len);
        return;
    }
    if (blockIdx.x == gridDim.x - 1) {                                       // the owner of len_attempts / len_accepts
        const int cells = a.R * a.M;
        for (int i = threadIdx.x; i < 2 * cells; i += STAT_BLOCK) s_len[i] = 0u;
        __syncthreads();
        for (int b = threadIdx.x; b < a.n; b += STAT_BLOCK) {
            int U;
            if (a.rng_mode == 1) U = pathlen_from_bits(philox4x32_10(U4{a.key.chain_lo + (uint32_t)b, (uint32_t)it, 0u, 0u}, a.key.k0, a.key.k1).x, a.pas);
            else U = a.U_in[b];
            U = min(max(U, 1), min(a.M, a.mu_cap));
            const int acc = ((const ChainRec*)(a.rec + (size_t)b * a.rec_stride))->acc_last;
            const int cell = stat_rung(a, it, b) * a.M + U - 1;
            atomicAdd(&s_len[cell], 1u);                                     // (LDS)
            if (acc) atomicAdd(&s_len[cells + cell], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += STAT_BLOCK) {
            const unsigned int at = s_len[i], ac = s_len[cells + i];
            if (at) a.len_attempts[i] += (long long)at;
            if (ac) a.len_accepts[i] += (long long)ac;
        }
        return;
    }
    const int b = __builtin_amdgcn_readfirstlane((int)((blockIdx.x - a.site_blocks) * STAT_NW + (threadIdx.x >> 6)));
    if (b >= a.n) return;
    const int lane = threadIdx.x & 63;
    const int nd = a.Ls >> 2;
    const ChainRec* rc = (const ChainRec*)(a.rec + (size_t)b * a.rec_stride);
    const int acc = rc->acc_last, dist = rc->dist_cur, dist_prev = a.pdist[b];
    const int r = stat_rung(a, it, b);
    const unsigned int* x = (const unsigned int*)(a.cur + (size_t)b * a.Ls);
    const unsigned int* p = (const unsigned int*)(prev + (size_t)b * a.Ls);
    unsigned int* o = (unsigned int*)(next + (size_t)b * a.Ls);
    int h = 0;
    for (int d = lane; d < nd; d += 64) {                                    // (Ls / 4 <= 78: at most two dwords per lane)
        const unsigned int v = x[d], w = p[d];
        const unsigned int df = (v ^ w) & arch_dword_mask(d, a.sh, a.L);
#pragma unroll
        for (int j = 0; j < 4; ++j) h += ((df >> (8 * j)) & 0xffu) ? 1 : 0;
        o[d] = v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) h += __shfl_xor(h, o);
    if (lane == 0) {
        const size_t c = (size_t)b * a.R + r;
        a.iters[c] += 1;
        if (acc) a.accepts[c] += 1;
        if (h > 0) { a.moved[c] += 1; a.jump_sum[c] += h; }
        if (dist) a.dist_sum[c] += dist;
        if (dist_prev > 0 && dist == 0) a.wt_returns[c] += 1;
        if (dist != dist_prev) a.pdist[b] = dist;
    }
}

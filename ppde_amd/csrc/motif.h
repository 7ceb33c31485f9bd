// Forbidden sequence patterns (ppde_chains_set_forbidden_patterns, include/ppde_hip.h): a constraint of the reversible chains'
// target, exp(E) 1[dist < thr] 1[x free] / Z. A state is free when no ACTIVE (pattern, start position) matches it; the host folds
// the patterns' lengths against L and the native exemption into active[L], one word per start position (bit m: pattern m is
// checked there).
//
// k_motif_veto runs once per iteration on the proposal slot, behind the proposal's expert evaluation and in front of the accept
// launch, and once inside a recombination event on the children (counters off). One wave per chain: a lane owns the start
// positions p, p + 64, ...: it loads the eight row bytes at sh + p + j once (independent loads, one round trip) and, for every set bit
// of active[p], tests the pattern's elements against them in registers (two 16-byte LDS reads per pattern, constant register indices).
// A wave minimum over (pattern << 16 | position) gives the lowest violated pattern and its lowest position. Lane 0 writes veto[b]
// (one byte, 0 or 1) and bumps the chain's own counter cell vetoes[b][pattern]: a chain belongs to one wave of one launch, so
// these are plain loads and stores. The REV accept kernels read veto[b] next to dist_prop (pas.h accept_body), k_cross_accept the
// two children's bytes. The kernel reads nothing that depends on the iteration index, so one launch is valid at every position of
// a captured segment and under eager issue.
//
// The patterns sit in LDS, [32][8] words: element j of pattern m at 8 m + j, 0 behind the pattern's length (an element inside it
// is never 0). k_motif_scan is the same device function over arbitrary rows (ppde_motif_scan).
#pragma once
#include "common.h"

#define MOTIF_MAX_PATTERNS 32
#define MOTIF_MAX_LEN 8
#define MOTIF_WORDS (MOTIF_MAX_PATTERNS * MOTIF_MAX_LEN)
#define MOTIF_BLOCK 256
#define MOTIF_NW (MOTIF_BLOCK / 64)
#define MOTIF_FREE 0x7fffffff

struct MotifArgs {
    const uint8_t* rows;        // row b at rows + b * stride, residue l at byte sh + l
    int stride, sh, L;
    int b_off, n_sub;           // rows [b_off, b_off + n_sub) of this launch
    int M;                      // patterns (the counters' row width)
    const uint32_t* active;     // [L]
    const uint32_t* pattern;    // [32][8]
    uint8_t* veto;              // [n]             (k_motif_veto)
    long long* vetoes;          // [n][M] or NULL  (k_motif_veto: NULL inside a recombination event)
    int* first_pattern;         // [n]             (k_motif_scan: -1 for a free row)
    int* first_pos;             // [n]
};

__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, dpp_i<DPP_XOR1>(v));
    v = min(v, dpp_i<DPP_XOR2>(v));
    v = min(v, dpp_i<DPP_HALF_MIRROR>(v));
    v = min(v, dpp_i<DPP_MIRROR>(v));
    v = min(v, dpp_rows_i<DPP_BCAST15, 0xA>(MOTIF_FREE, v));
    v = min(v, dpp_rows_i<DPP_BCAST31, 0xC>(MOTIF_FREE, v));
    return __builtin_amdgcn_readlane(v, 63);
}

// the [32][8] element words into LDS, a pattern's eight words as two uint4
__device__ __forceinline__ void motif_stage(const MotifArgs& a, uint4* pat) {
    if (threadIdx.x < MOTIF_WORDS / 4) pat[threadIdx.x] = ((const uint4*)a.pattern)[threadIdx.x];
    __syncthreads();
}
// letter x lies in element e, or e is one of the zero words behind the pattern's length
__device__ __forceinline__ bool motif_in(uint32_t e, uint32_t x) { return (e == 0u) | (((e >> x) & 1u) != 0u); }

// (lowest violated pattern << 16) | its lowest position, or MOTIF_FREE; the same value in every lane of the wave
__device__ __forceinline__ int motif_first(const MotifArgs& a, const uint4* pat, const uint8_t* row) {
    const int lane = threadIdx.x & 63;
    int key = MOTIF_FREE;
    for (int p = lane; p < a.L; p += 64) {
        uint32_t act = a.active[p];
        if (!act) continue;
        // an active bit promises p + len <= L: the bytes behind the row's end (index clamped) meet zero words only
        uint32_t x[MOTIF_MAX_LEN];
#pragma unroll
        for (int j = 0; j < MOTIF_MAX_LEN; ++j) x[j] = row[a.sh + min(p + j, a.L - 1)] & 31u;
        while (act) {
            const int m = __builtin_ctz(act);
            act &= act - 1;
            const uint4 e0 = pat[2 * m], e1 = pat[2 * m + 1];
            const bool hit = motif_in(e0.x, x[0]) & motif_in(e0.y, x[1]) & motif_in(e0.z, x[2]) & motif_in(e0.w, x[3]) &
                             motif_in(e1.x, x[4]) & motif_in(e1.y, x[5]) & motif_in(e1.z, x[6]) & motif_in(e1.w, x[7]);
            if (hit) key = min(key, (m << 16) | p);
        }
    }
    return wave_min_i(key);
}

__global__ __launch_bounds__(MOTIF_BLOCK) void k_motif_veto(MotifArgs a) {
    __shared__ uint4 pat[MOTIF_WORDS / 4];
    motif_stage(a, pat);
    const int w = blockIdx.x * MOTIF_NW + (threadIdx.x >> 6);
    if (w >= a.n_sub) return;
    const int b = a.b_off + w;
    const int key = motif_first(a, pat, a.rows + (size_t)b * a.stride);
    if ((threadIdx.x & 63) == 0) {
        a.veto[b] = key != MOTIF_FREE ? 1 : 0;
        if (key != MOTIF_FREE && a.vetoes) a.vetoes[(size_t)b * a.M + (key >> 16)] += 1;
    }
}

__global__ __launch_bounds__(MOTIF_BLOCK) void k_motif_scan(MotifArgs a) {
    __shared__ uint4 pat[MOTIF_WORDS / 4];
    motif_stage(a, pat);
    const int w = blockIdx.x * MOTIF_NW + (threadIdx.x >> 6);
    if (w >= a.n_sub) return;
    const int b = a.b_off + w;
    const int key = motif_first(a, pat, a.rows + (size_t)b * a.stride);
    if ((threadIdx.x & 63) == 0) {
        a.first_pattern[b] = key != MOTIF_FREE ? key >> 16 : -1;
        a.first_pos[b] = key != MOTIF_FREE ? key & 0xffff : -1;
    }
}

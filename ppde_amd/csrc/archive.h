// Archive of each chain's K best distinct sequences (ppde_chains_set_archive, include/ppde_hip.h).
//
// k_archive is launched behind the accept phase (and behind k_swap, when there is one) of EVERY iteration of an archiving run, and
// once by ppde_chains_init for t = 0. The iteration index is the device counter + the node-local offset, as in k_record, so a
// captured graph segment is valid at any offset. The candidate of chain b after t completed iterations is what ppde_chains_peek
// returns: the state row of `cur` with row t of the two histories (untempered).
//   skipped, before anything else: ChainRec::dist_cur == 0 (the wild type; in the default mode also the iteration of a mutation-cap
//     reset, whose history row holds the energy of the state that was reset away), and an energy that is not finite;
//   1. an archived entry with the same L letters: nothing happens (the entry keeps its first energy and step);
//   2. else count < K: inserted with step = t;
//   3. else m = the entry of lowest energy, the latest step among equal energies; replaced when e > energy[m] (strict).
// One wave owns one chain, four chains per workgroup. Lanes are the dwords of the state row (Ls / 4 <= 78: a lane holds at most
// two); lanes 0 .. K-1 hold the entries' energies and steps for the eviction arg-min, a fixed butterfly on the key
// (energy ascending, step descending). Steps are unique within a chain, so the minimum is unique. Entry rows are kept in the
// state-row layout [n][K][Ls]; ppde_chains_archive_read unpacks them with k_unpack_state. Pad bytes outside [sh, sh + L) are
// masked out of every comparison. Every entry carries a 32-bit fingerprint of its residue bytes; the duplicate test reads only
// the rows whose fingerprint equals the candidate's (usually none or one), and an entry is a duplicate only after its bytes were
// compared. The loads behind the three exits -- dist_cur, count, the K energies, steps and fingerprints, history row t -- are
// issued before the first branch, so the steady state (a full archive, a candidate that does not beat the minimum) costs two
// memory round trips and touches no state byte.
// No wave reads or writes another chain's archive, there are no atomics, no LDS, and nothing a wave reads is written by another
// thread of the launch (k_swap's rule): a wave reads its own entries and then writes one of them.
#pragma once
#include "common.h"
#include "pas.h"

#define ARCH_BLOCK 256
#define ARCH_KMAX 32

struct ArchArgs {
    const int* it_base;         // device iteration base (graph replay) or NULL
    int it_local;               // t = base + it_local + 1 (ppde_chains_init passes -1)
    int n, K, L, Ls, sh;        // chains, entries per chain, residues, state-row stride, byte of residue 0
    int rec_stride;
    const unsigned char* rec;   // [n] chain records (ChainRec::dist_cur)
    const uint8_t* cur;         // [n][Ls]
    const float* e_hist;        // [T+1][n]
    const float* f_hist;
    uint8_t* idx;               // [n][K][Ls]
    float* energy;              // [n][K]
    float* fitness;
    int* step;
    unsigned int* hash;         // [n][K] fingerprint of the entry's residue bytes
    int* count;                 // [n]
};

// bytes of dword d of a state row that are residues: 0xff per byte inside [sh, sh + L)
__device__ __forceinline__ unsigned int arch_dword_mask(int d, int sh, int L) {
    unsigned int m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = 4 * d + j - sh;
        m |= (l >= 0 && l < L) ? (0xffu << (8 * j)) : 0u;
    }
    return m;
}

__global__ __launch_bounds__(ARCH_BLOCK) void k_archive(ArchArgs a) {
    typedef const __attribute__((address_space(4))) int* cptr;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ARCH_BLOCK / 64) + (threadIdx.x >> 6)));
    if (b >= a.n) return;
    const int lane = threadIdx.x & 63;
    const int K = a.K;
    const size_t eb = (size_t)b * K;
    // every load that does not need the iteration index goes out together with the scalar load of the counter: the exits below
    // are decided after two memory round trips (the counter, then history row t), not one per condition
    const int base = a.it_base ? *(cptr)(a.it_base) : 0;
    const int dist = ((const ChainRec*)(a.rec + (size_t)b * a.rec_stride))->dist_cur;
    const int cnt_v = a.count[b];
    const bool mine = lane < K;                                              // (all K cells exist, whatever count says)
    float ke = mine ? a.energy[eb + lane] : INFINITY;
    int ks = mine ? a.step[eb + lane] : -1;
    const unsigned int kh = mine ? a.hash[eb + lane] : 0u;
    const int t = base + a.it_local + 1;                                     // completed iterations
    const float e = a.e_hist[(size_t)t * a.n + b];
    const int cnt = min(__builtin_amdgcn_readfirstlane(cnt_v), K);
    const bool live = lane < cnt;
    ke = live ? ke : INFINITY;                                               // (a lane without an entry never wins: K >= 1)
    ks = live ? ks : -1;
    int ki = lane;
#pragma unroll
    for (int o = 1; o < ARCH_KMAX; o <<= 1) {                                // arg-min of (energy ascending, step descending)
        const float oe = __shfl_xor(ke, o);
        const int os = __shfl_xor(ks, o), oi = __shfl_xor(ki, o);
        const bool take = oe < ke || (oe == ke && os > ks);
        ke = take ? oe : ke; ks = take ? os : ks; ki = take ? oi : ki;
    }
    const float emin = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ke)));
    const bool full = cnt >= K;
    // wave-uniform exits: the wild type; NaN, +inf, -inf; the steady state (a full archive, no gain), which touches no state byte
    if (dist == 0 || !(fabsf(e) < INFINITY) || (full && !(e > emin))) return;
    const int m = full ? __builtin_amdgcn_readfirstlane(ki) : cnt;           // the entry to write: the minimum, or the next free one
    // the candidate's row: dwords lane and lane + 64, and its fingerprint over the residue bytes
    const int nd = a.Ls >> 2;
    const bool h0 = lane < nd, h1 = lane + 64 < nd;
    const unsigned int* src = (const unsigned int*)(a.cur + (size_t)b * a.Ls);
    const unsigned int m0 = h0 ? arch_dword_mask(lane, a.sh, a.L) : 0u, m1 = h1 ? arch_dword_mask(lane + 64, a.sh, a.L) : 0u;
    const unsigned int v0 = (h0 ? src[lane] : 0u) & m0, v1 = (h1 ? src[lane + 64] : 0u) & m1;
    unsigned int hc = (v0 ^ ((unsigned int)lane * 0x27D4EB2Fu)) * 0x9E3779B1u;
    hc ^= hc >> 15;
    hc += (v1 ^ ((unsigned int)(lane + 64) * 0x165667B1u)) * 0x85EBCA77u;
    hc ^= hc >> 13;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) hc ^= __shfl_xor(hc, o);
    // duplicate test: only entries with the candidate's fingerprint are compared, and an entry is a duplicate only by its bytes
    unsigned int* rows = (unsigned int*)(a.idx + eb * a.Ls);
    unsigned long long cand = __ballot(live && kh == hc);
    bool dup = false;
    while (cand) {                                                           // (wave-uniform: a ballot)
        const int j = __ffsll((long long)cand) - 1;
        cand &= cand - 1;
        const unsigned int* r = rows + (size_t)j * nd;
        const unsigned int w0 = (h0 ? r[lane] : 0u) & m0, w1 = (h1 ? r[lane + 64] : 0u) & m1;
        dup = dup || __ballot(((v0 ^ w0) | (v1 ^ w1)) != 0u) == 0ull;
    }
    if (dup) return;
    unsigned int* dst = rows + (size_t)m * nd;
    if (h0) dst[lane] = v0;                                                  // (pad bytes are stored as zero)
    if (h1) dst[lane + 64] = v1;
    if (lane == 0) {
        a.energy[eb + m] = e;
        a.fitness[eb + m] = a.f_hist[(size_t)t * a.n + b];
        a.step[eb + m] = t;
        a.hash[eb + m] = hc;
        if (!full) a.count[b] = cnt + 1;
    }
}

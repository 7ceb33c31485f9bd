// Pairwise letter co-occurrence counts of the recorded samples (ppde_chains_set_pair_counts, include/ppde_hip.h).
//
// k_record_pairs is launched directly behind k_record in every iteration of a run that has pair counts, with k_record's schedule:
// the iteration is the device counter + the node-local offset, and an iteration that is not recorded leaves through a
// launch-uniform branch after that one scalar load. It reads `cur` (and slot[e][rung] when the recorder follows a rung), never the
// sample buffer, so a counts-only recorder has pair counts too.
//   pair_counts[i][a][j][b] = number of recorded (row, slot) pairs with letter a at residue sites[i] and letter b at sites[j].
// One workgroup owns one tile of PAIR_TS x PAIR_TS site pairs, tile row <= tile column (the lower block triangle is the mirror
// image and is filled on read): PAIR_TS^2 pairs x 400 letter pairs of uint32 bins in LDS. Lanes are slots: a thread loads its
// slot's 2 PAIR_TS letters from the state row and issues PAIR_TS^2 LDS atomic adds without return; integer adds commute, so the
// result does not depend on the order (the route phase of cnn.h relies on the same). After one barrier every bin has one owning
// thread, which does a plain 64-bit load, add and store into the tile's block of the device array, and skips an increment of
// zero. Every global counter has exactly one owner per launch, there are no global atomics, and no thread reads what another
// thread of the launch writes (k_swap's and k_record's rule). The site list is padded with -1 to whole tiles: a ragged last tile
// tests its sites once, uniformly over the workgroup.
// Device layout: [tile (ti <= tj), row-major over the upper triangle][p * PAIR_TS + q][20 a + b], site i = PAIR_TS ti + p,
// site j = PAIR_TS tj + q. A diagonal tile holds all its PAIR_TS^2 pairs, both orders.
#pragma once
#include "common.h"

#define PAIR_BLOCK 256
#define PAIR_TS 4
#define PAIR_BINS (PPDE_A * PPDE_A)
#define PAIR_TILE (PAIR_TS * PAIR_TS * PAIR_BINS)       // bins of one tile: 6400 (25.6 KB of LDS)

struct PairArgs {
    const int* it_base;         // device iteration base (graph replay) or NULL
    int it_local;
    int Ls, sh;                 // state-row stride, byte of residue 0
    int burn_in, every;
    int rung, n_rungs;          // rung < 0: every chain is a slot; else slot e = slot[e][rung]
    int slots;
    int nt;                     // tiles per side = ceil(S / PAIR_TS); the grid has nt (nt + 1) / 2 workgroups
    const uint8_t* cur;         // [n][Ls]
    const int* slot;            // [n/R][R] rung -> chain (tempering), or NULL
    const int* sites;           // [nt * PAIR_TS] residues, strictly increasing, padded with -1
    unsigned long long* counts; // [nt (nt + 1) / 2][PAIR_TILE]
};

__global__ __launch_bounds__(PAIR_BLOCK) void k_record_pairs(PairArgs a) {
    typedef const __attribute__((address_space(4))) int* cptr;
    const int t = (a.it_base ? *(cptr)(a.it_base) : 0) + a.it_local + 1;     // completed iterations
    const int d = t - a.burn_in;
    if (d <= 0 || d % a.every != 0) return;                                  // (uniform over the launch)

    __shared__ unsigned int s_bin[PAIR_TILE];
    int ti = 0, rem = blockIdx.x;                                            // tile (ti, tj) of the upper triangle, row-major
    while (rem >= a.nt - ti) { rem -= a.nt - ti; ++ti; }
    const int tj = ti + rem;
    int off_i[PAIR_TS], off_j[PAIR_TS];                                      // byte of each site in a state row, or -1 (ragged tile)
#pragma unroll
    for (int p = 0; p < PAIR_TS; ++p) {
        const int si = a.sites[ti * PAIR_TS + p], sj = a.sites[tj * PAIR_TS + p];
        off_i[p] = si >= 0 ? a.sh + si : -1;
        off_j[p] = sj >= 0 ? a.sh + sj : -1;
    }
    for (int i = threadIdx.x; i < PAIR_TILE; i += PAIR_BLOCK) s_bin[i] = 0u;
    __syncthreads();

    for (int s = threadIdx.x; s < a.slots; s += PAIR_BLOCK) {
        const int ch = a.rung >= 0 ? a.slot[(size_t)s * a.n_rungs + a.rung] : s;
        const uint8_t* row = a.cur + (size_t)ch * a.Ls;
        unsigned int la[PAIR_TS], lb[PAIR_TS];
#pragma unroll
        for (int p = 0; p < PAIR_TS; ++p) {
            la[p] = off_i[p] >= 0 ? row[off_i[p]] : 0xffu;                   // (0xff is no letter: no bin)
            lb[p] = off_j[p] >= 0 ? row[off_j[p]] : 0xffu;
        }
#pragma unroll
        for (int p = 0; p < PAIR_TS; ++p)
#pragma unroll
            for (int q = 0; q < PAIR_TS; ++q)
                if (la[p] < (unsigned)PPDE_A && lb[q] < (unsigned)PPDE_A)
                    atomicAdd(&s_bin[(p * PAIR_TS + q) * PAIR_BINS + la[p] * PPDE_A + lb[q]], 1u);
    }
    __syncthreads();
    unsigned long long* blk = a.counts + (size_t)blockIdx.x * PAIR_TILE;
    for (int i = threadIdx.x; i < PAIR_TILE; i += PAIR_BLOCK) {              // the owner of bin i of this tile
        const unsigned int v = s_bin[i];
        if (v) blk[i] += (unsigned long long)v;
    }
}

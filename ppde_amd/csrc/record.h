// Recorder of thinned population samples and per-site letter counts (ppde_chains_set_recorder, include/ppde_hip.h).
//
// k_record is launched behind the accept phase (and behind k_swap, when there is one) of EVERY iteration of a recording run, so a
// captured graph segment is valid at any offset: the iteration index is the device counter + the node-local offset, as in the
// chain kernels, and an iteration that is not recorded leaves through a wave-uniform branch after that one scalar load.
//   recorded: t = it + 1 completed iterations with t > burn_in and (t - burn_in) % every == 0, into row (t - burn_in) / every - 1;
//   slots: every chain (rung < 0), or one per tempering ensemble = the chain that holds `rung` after this iteration's swap;
//   a row = what ppde_chains_peek returns after that iteration: the state rows of `cur` (post-reset), row t of the histories.
// One workgroup owns 16 bytes (four dwords) of the state row, lanes are slots. State rows are Ls bytes apart, Ls a multiple of 4
// with an ODD number of dwords (set_geom in ppde_api.hip: distinct LDS banks for strided reads), so a row starts on a 4-byte
// boundary only: a slot's piece is copied as up to four aligned dword loads and stores (the last workgroup owns the ragged end),
// into samples kept in the same state-row layout [rows][slots][Ls]; ppde_chains_recorder_read unpacks them with k_unpack_state.
// Counts: per byte and letter one ballot + population count per wave, lane k keeping letter k's total in a register; the waves
// are merged in LDS and the owning thread of each (residue, letter) then does a plain 64-bit load, add and store. Every global
// counter has exactly one owner per launch, there are no global atomics, and no thread reads what another thread of the launch
// writes (k_swap's rule). Pad bytes are never counted. Energy, fitness and chain rows are written by the first workgroup.
#pragma once
#include "common.h"

#define REC_BLOCK 256
#define REC_NW (REC_BLOCK / 64)

struct RecArgs {
    const int* it_base;         // device iteration base (graph replay) or NULL
    int it_local;
    int n, L, Ls, sh;           // chains in the buffers, residues, state-row stride, byte of residue 0
    int burn_in, every;
    int rung, n_rungs;          // rung < 0: every chain is a slot; else slot e = slot[e][rung]
    int slots;
    const uint8_t* cur;         // [n][Ls]
    const float* e_hist;        // [T+1][n]
    const float* f_hist;
    const int* slot;            // [n/R][R] rung -> chain (tempering), or NULL
    uint8_t* idx;               // [rows][slots][Ls], or NULL (counts only)
    float* energy;              // [rows][slots], or NULL
    float* fitness;
    int* chain;
    unsigned long long* counts; // [L][20]
};

__global__ __launch_bounds__(REC_BLOCK) void k_record(RecArgs a) {
    typedef const __attribute__((address_space(4))) int* cptr;
    const int t = (a.it_base ? *(cptr)(a.it_base) : 0) + a.it_local + 1;     // completed iterations
    const int d = t - a.burn_in;
    if (d <= 0 || d % a.every != 0) return;                                  // (uniform over the launch)
    const int row = d / a.every - 1;

    __shared__ unsigned int s_cnt[REC_NW][16][PPDE_A];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wg = blockIdx.x;
    const int nd = a.Ls >> 2;                                                // dwords of a state row
    const int d0 = 4 * wg;                                                   // first dword this workgroup owns
    const int l0 = 16 * wg - a.sh;                                           // residue of its first byte

    unsigned int cnt[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) cnt[j] = 0u;

    for (int base = w * 64; base < a.slots; base += REC_BLOCK) {             // (wave-uniform trip count)
        const int s = base + lane;
        const bool live = s < a.slots;
        unsigned int v[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};   // (0xff matches no letter)
        if (live) {
            const int ch = a.rung >= 0 ? a.slot[(size_t)s * a.n_rungs + a.rung] : s;
            const unsigned int* src = (const unsigned int*)(a.cur + (size_t)ch * a.Ls) + d0;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (d0 + j < nd) v[j] = src[j];
            const size_t o = (size_t)row * a.slots + s;
            if (a.idx) {
                unsigned int* dst = (unsigned int*)(a.idx + o * a.Ls) + d0;
#pragma unroll
                for (int j = 0; j < 4; ++j) if (d0 + j < nd) dst[j] = v[j];
            }
            if (wg == 0 && a.energy) {
                a.energy[o] = a.e_hist[(size_t)t * a.n + ch];
                a.fitness[o] = a.f_hist[(size_t)t * a.n + ch];
                a.chain[o] = ch;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int l = l0 + j;
            if (l < 0 || l >= a.L) continue;                                 // pad byte (uniform over the workgroup)
            const unsigned int letter = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
#pragma unroll
            for (int k = 0; k < PPDE_A; ++k) {
                const unsigned int c = (unsigned int)__popcll(__ballot(letter == (unsigned int)k));
                cnt[j] += lane == k ? c : 0u;
            }
        }
    }
    if (lane < PPDE_A) {
#pragma unroll
        for (int j = 0; j < 16; ++j) s_cnt[w][j][lane] = cnt[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * PPDE_A; i += REC_BLOCK) {             // the owner of (residue, letter)
        const int j = i / PPDE_A, k = i - j * PPDE_A, l = l0 + j;
        if (l < 0 || l >= a.L) continue;
        unsigned int sum = 0u;
#pragma unroll
        for (int q = 0; q < REC_NW; ++q) sum += s_cnt[q][j][k];
        a.counts[(size_t)l * PPDE_A + k] += (unsigned long long)sum;
    }
}

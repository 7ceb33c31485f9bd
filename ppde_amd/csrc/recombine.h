// Recombination (ppde_chains_set_recombination, include/ppde_hip.h): a segment exchange between two chains of a deme, as a
// Metropolis move on the pair (the crossover of evolutionary Monte Carlo, Liang & Wong 2000).
//
// The HOST decides which iterations are events ((it + 1) % every == 0, event s = (it + 1) / every - 1) and launches, behind the
// plain accept kernel of such an iteration only: k_cross_propose, the run's expert evaluation of the proposal slot, k_cross_accept.
// The kernels take the iteration index from the device counter + the node-local offset like every other kernel, so a captured
// segment is valid at any position that is a multiple of `every`; they re-derive s and return when the iteration is no event.
//
// Pairing (circle method): m = D - 1, r = s mod m; pair 0 of a deme is (r, m), pair k >= 1 is ((r + k) mod m, (r - k) mod m) --
// slot i < m, i != r meets (2r - i) mod m. The lower slot is `a`. One Philox draw per pair at (global index of a, it, 0x40000002, 0):
// i1 = mulhi(x, S_o), i2 = mulhi(y, S_o), the segment = the open residues open[min(i1, i2) .. max(i1, i2)], u = unif_from_bits(z).
//
// k_cross_propose: one 256-thread workgroup per pair. Reads both current rows, writes both children's WHOLE rows (padding bytes
//   of the own parent) into the proposal state and the whole padded Potts window into its T4 copy (the slot holds a stale PAS
//   proposal), counts differ and the two child_dist (wave reductions, one LDS exchange) and writes the record row's
//   partner / lo / hi / differ / child_dist / pre_energy.
// k_cross_accept: one workgroup per pair. Decision in fp32: d = (E'_a - E_a) + (E'_b - E_b); outcome 3 a non-finite child energy,
//   2 a child at or over the mutation cap, 4 a child that matches a forbidden pattern (none goes through u), 1 expf(d) >= u, 0
//   otherwise. An accepted pair's two slots take
//   from the proposal slot what k_select_copy gives a replaced slot: state row + T4 bytes, cur_e / cur_f / dist_cur, the grad_cur
//   row under gradient reuse (the combined row of slot 1), row it + 1 of both histories (and of rtraj), the running best by the
//   accept phase's strict rule. The last accept bit and the traces stay the slot's own Metropolis result.
// A workgroup touches its own two slots only: no workgroup reads what another of the same launch writes. No global atomics;
// every global write is a plain store.
#pragma once
#include "common.h"
#include "pas.h"

#define CROSS_BLOCK 256
#define CROSS_NW (CROSS_BLOCK / 64)
#define CROSS_STREAM 0x40000002u

struct CrossArgs {
    PasArgs p;                  // the object's chain arguments (it_base / it_local of the event's iteration)
    int D, every, cap, n_open;  // deme size, iterations per event, events_cap, open residues
    const int* open;            // [n_open] the open list, increasing
    int* partner;               // [events_cap][n] each
    int* lo;
    int* hi;
    int* differ;
    int* child_dist;
    uint8_t* outcome;
    float* log_ratio;
    float* pre_energy;
    float* child_energy;
};

// event behind iteration `it`, or -1
__device__ __forceinline__ int cross_event(const CrossArgs& a, int& it) {
    typedef const __attribute__((address_space(4))) int* cptr;
    it = (a.p.it_base ? *(cptr)(a.p.it_base) : 0) + a.p.it_local;
    if ((it + 1) % a.every != 0) return -1;
    const int s = (it + 1) / a.every - 1;
    return s < a.cap ? s : -1;
}

// local chain indices (la < lb) of pair `q` of the object at event s
__device__ __forceinline__ void cross_pair(const CrossArgs& a, int s, int q, int& la, int& lb) {
    const int half = a.D >> 1, m = a.D - 1, r = s % m;
    const int deme = q / half, k = q - deme * half;
    const int i = k == 0 ? r : (r + k) % m, j = k == 0 ? m : (r - k + m) % m;
    la = deme * a.D + min(i, j);
    lb = deme * a.D + max(i, j);
}

struct CrossDraw { int lo, hi; float u; };
__device__ __forceinline__ CrossDraw cross_draw(const CrossArgs& a, int la, int it) {
    const U4 r = philox4x32_10(U4{a.p.key.chain_lo + (uint32_t)la, (uint32_t)it, CROSS_STREAM, 0u}, a.p.key.k0, a.p.key.k1);
    const int i1 = (int)__umulhi(r.x, (uint32_t)a.n_open), i2 = (int)__umulhi(r.y, (uint32_t)a.n_open);
    CrossDraw d;
    d.lo = min(i1, i2); d.hi = max(i1, i2);
    d.u = unif_from_bits(r.z);
    return d;
}

__global__ __launch_bounds__(CROSS_BLOCK) void k_cross_propose(CrossArgs a) {
    int it;
    const int s = cross_event(a, it);
    if (s < 0) return;
    __shared__ float xs[3 * CROSS_NW];
    const PasArgs& p = a.p;
    const Geom g = p.g;
    const int tid = threadIdx.x;
    int la, lb;
    cross_pair(a, s, blockIdx.x, la, lb);
    const CrossDraw dr = cross_draw(a, la, it);
    const int l_lo = a.open[dr.lo], l_hi = a.open[dr.hi];
    const uint8_t* ra = p.cur + (size_t)la * g.Ls;
    const uint8_t* rb = p.cur + (size_t)lb * g.Ls;
    uint8_t* pa = p.prop + (size_t)la * g.Ls;
    uint8_t* pb = p.prop + (size_t)lb * g.Ls;
    int nd = 0, da = 0, db = 0;
    for (int k = tid; k < g.Ls; k += CROSS_BLOCK) {
        const uint8_t va = ra[k], vb = rb[k];
        const int l = k - g.sh;
        const bool in_row = l >= 0 && l < g.L;
        const bool seg = in_row && l >= l_lo && l <= l_hi && (!p.allowed || p.allowed[l] != 0u);
        const uint8_t ca = seg ? vb : va, cb = seg ? va : vb;
        pa[k] = ca;
        pb[k] = cb;
        if (in_row) {
            const uint8_t w = p.wt[k];
            da += ca != w ? 1 : 0;
            db += cb != w ? 1 : 0;
            nd += (seg && va != vb) ? 1 : 0;
        }
    }
    if (g.Lp > 0)                                    // the padded Potts window's bytes, at store_letter's addresses
        for (int wl = tid; wl < 16 * g.NC; wl += CROSS_BLOCK) {
            const size_t oa = state_t4_offset_dev(g.NC, p.n_pad, la, wl), ob = state_t4_offset_dev(g.NC, p.n_pad, lb, wl);
            const int l = g.i0 + wl;
            const bool seg = l < g.L && l >= l_lo && l <= l_hi && (!p.allowed || p.allowed[l] != 0u);
            // an exchanged residue takes the other parent's letter (what store_letter would write), everything else the own byte
            p.propT[oa] = seg ? rb[g.sh + l] : p.curT[oa];
            p.propT[ob] = seg ? ra[g.sh + l] : p.curT[ob];
        }
    // counts below 2^24: exact in fp32
    const float snd = wave_sum((float)nd), sda = wave_sum((float)da), sdb = wave_sum((float)db);
    if ((tid & 63) == 0) { xs[tid >> 6] = snd; xs[CROSS_NW + (tid >> 6)] = sda; xs[2 * CROSS_NW + (tid >> 6)] = sdb; }
    __syncthreads();
    if (tid == 0) {
        float tn = 0.f, ta = 0.f, tb = 0.f;
#pragma unroll
        for (int w = 0; w < CROSS_NW; ++w) { tn += xs[w]; ta += xs[CROSS_NW + w]; tb += xs[2 * CROSS_NW + w]; }
        const size_t row = (size_t)s * p.n, hrow = (size_t)(it + 1) * p.n;
        a.partner[row + la] = lb; a.partner[row + lb] = la;
        a.lo[row + la] = dr.lo; a.lo[row + lb] = dr.lo;
        a.hi[row + la] = dr.hi; a.hi[row + lb] = dr.hi;
        a.differ[row + la] = (int)tn; a.differ[row + lb] = (int)tn;
        a.child_dist[row + la] = (int)ta; a.child_dist[row + lb] = (int)tb;
        a.pre_energy[row + la] = p.e_hist[hrow + la];
        a.pre_energy[row + lb] = p.e_hist[hrow + lb];
    }
}

// slot d takes its child from the proposal slot (k_select_copy's writes with sources in slot 1)
__device__ __forceinline__ void cross_take(const CrossArgs& a, int d, float e, float f, int dist, int it) {
    const PasArgs& p = a.p;
    const Geom g = p.g;
    const int tid = threadIdx.x;
    if (p.reuse) {
        const RowSrc r = slot_row(p, 1, d);
        float4* dst = (float4*)(p.grad_cur + (size_t)d * g.N);
        for (int k = tid; k < g.N / 4; k += CROSS_BLOCK) dst[k] = row_value(r, k);
    }
    {
        const uint32_t* src = (const uint32_t*)(p.prop + (size_t)d * g.Ls);
        uint32_t* dst = (uint32_t*)(p.cur + (size_t)d * g.Ls);
        for (int k = tid; k < g.Ls / 4; k += CROSS_BLOCK) dst[k] = src[k];
    }
    if (g.Lp > 0)
        for (int wl = tid; wl < 16 * g.NC; wl += CROSS_BLOCK) {
            const size_t o = state_t4_offset_dev(g.NC, p.n_pad, d, wl);
            p.curT[o] = p.propT[o];
        }
    if (tid < 64) {
        ChainRec* rd = (ChainRec*)(p.rec + (size_t)d * p.rec_stride);
        const bool better = e > rd->best_e;          // strict, like the accept phase
        const bool traj = d == p.random_chain;
        if (better || traj)
            for (int l = tid; l < g.L; l += 64) {
                const uint8_t v = p.prop[(size_t)d * g.Ls + g.sh + l];
                if (better) p.best_state[(size_t)d * g.L + l] = v;
                if (traj) p.rtraj[(size_t)(it + 1) * g.L + l] = v;
            }
        if (tid == 0) {
            const size_t hrow = (size_t)(it + 1) * p.n;
            p.e_hist[hrow + d] = e;
            p.f_hist[hrow + d] = f;
            rd->cur_e = e; rd->cur_f = f; rd->dist_cur = dist;
            if (better) { rd->best_e = e; rd->best_f = f; rd->best_t = it + 1; }
        }
    }
}

__global__ __launch_bounds__(CROSS_BLOCK) void k_cross_accept(CrossArgs a) {
    int it;
    const int s = cross_event(a, it);
    if (s < 0) return;
    const PasArgs& p = a.p;
    const int tid = threadIdx.x;
    int la, lb;
    cross_pair(a, s, blockIdx.x, la, lb);
    const CrossDraw dr = cross_draw(a, la, it);
    const size_t row = (size_t)s * p.n;
    // every wave computes the same values
    float ea, fa, eb, fb;
    slot_energy(p, 1, la, ea, fa);
    slot_energy(p, 1, lb, eb, fb);
    const float Ea = a.pre_energy[row + la], Eb = a.pre_energy[row + lb];
    const int da = a.child_dist[row + la], db = a.child_dist[row + lb];
    const float d = (ea - Ea) + (eb - Eb);
    const bool finite = fabsf(ea) < INFINITY && fabsf(eb) < INFINITY;    // (false for NaN and both infinities)
    int outcome;
    if (!finite) outcome = 3;
    else if (da >= p.thr || db >= p.thr) outcome = 2;                    // (thr = INT_MAX without a cap)
    else if (p.veto && (p.veto[la] | p.veto[lb])) outcome = 4;           // a child is not free (motif.h)
    else outcome = expf(d) >= dr.u ? 1 : 0;
    if (tid == 0) {
        a.outcome[row + la] = (uint8_t)outcome; a.outcome[row + lb] = (uint8_t)outcome;
        a.log_ratio[row + la] = d; a.log_ratio[row + lb] = d;
        a.child_energy[row + la] = ea; a.child_energy[row + lb] = eb;
    }
    if (outcome != 1) return;
    cross_take(a, la, ea, fa, da, it);
    cross_take(a, lb, eb, fb, db, it);
}

// Host side of the C ABI declared in include/ppde_hip.h, the one translation unit of the library. Here: device memory ownership,
// the model and its weight re-layout, the expert launch layer, ppde_energy_grad. The chains object (ppde_chains_*, hipGraph capture
// and replay of the iteration loop) is in chains.h and the *_host.h it includes, at the end of this file.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/ppde_hip.h"
#include "common.h"
#include "potts.h"
#include "cnn.h"
#include "pas.h"
#include "record.h"
#include "pairs.h"
#include "archive.h"
#include "stats.h"
#include "anneal.h"
#include "recombine.h"
#include "motif.h"

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
// The environment knobs (tuning and diagnostics) are read here and nowhere else; every site keeps its value in a function-local
// static, so a knob is read once per process, at its first use. Unset: nullptr / the default.
static const char* env_str(const char* name) { return getenv(name); }
static int env_int(const char* name, int dflt) {
    const char* e = env_str(name);
    return e ? atoi(e) : dflt;
}
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            return fail(PPDE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));              \
    } while (0)
#define ARGCHK(c, msg)                                                                              \
    do {                                                                                            \
        if (!(c)) return fail(PPDE_ERR_INVALID, std::string(msg));                                  \
    } while (0)

template <typename T>
static hipError_t dalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    return hipMalloc((void**)p, count * sizeof(T));
}

// The one owner of a device allocation in this file: a mode's buffers as members of its struct (Tempering ... MoveStats below), a
// call's temporaries as locals. Move-only; every way out of a scope (HIPCHK / ARGCHK included) releases what it holds, and
// assigning over one releases what was there. Reads as the plain pointer wherever one is expected.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { if (p) hipFree(p); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t count) {                 // (dalloc's rule: a count of 0 allocates one element)
        if (p) hipFree(p);
        return dalloc(&p, count);
    }
    hipError_t alloc_zero(size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T));
    }
    operator T*() const { return p; }
};

#include "tf_host.h"

// Scope guard for the event pairs of the timing hooks: every early return (HIPCHK / ARGCHK) releases them.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

// --------------------------------------------------------------------------------------------
struct ppde_model {
    int device = 0;
    int L = 0;
    Geom g{};
    std::vector<uint8_t> h_wt;       // plain [L]
    uint8_t* d_wt = nullptr;         // state layout [Ls]
    uint32_t* d_wtT = nullptr;       // its T4 copy (potts.h), for one chain
    // Potts
    bool has_potts = false;
    float4* d_Jt = nullptr;
    float* d_h = nullptr;
    float wt_H = 0.f;
    // CNN
    bool has_cnn = false;
    int n_nets = 0, C = 0, CP = 0, K = 0, KT = 0, F = 0, FP = 0, T = 0, J = 0, JP = 0;
    CnnNet nets[4]{};
    std::vector<void*> cnn_allocs;
    float lamda = 0.f;
    // scratch of the stateless API
    int scratch_n = 0;
    uint8_t* s_state = nullptr;
    uint32_t* s_stateT = nullptr;
    float *s_grad = nullptr, *s_epart = nullptr, *s_gradC = nullptr, *s_fitC = nullptr;
    int* s_flag = nullptr;
    // transformer expert (tf_host.h) and the stateless API's workspace for it
    TfModel* tf = nullptr;
    TfWork* s_tfw = nullptr;
    float *s_gradT = nullptr, *s_tfE = nullptr;
    int s_tf_n = 0;                  // chains s_gradT / s_tfE are sized for
    // chunk maxima of the long-sequence CNN path, sized for `cnn_scratch_n` chains
    float* cnn_cmax = nullptr;
    int* cnn_carg = nullptr;
    uint32_t* cnn_cgate = nullptr;   // ReLU gate bits of h1, written by the forward chunks for the backward chunks
    int cnn_scratch_n = 0;
};

static void set_geom(ppde_model* m, int Lp, int i0) {
    Geom& g = m->g;
    g.L = m->L;
    g.N = m->L * PPDE_A;
    g.Lp = Lp;
    g.i0 = i0;
    g.NC = Lp > 0 ? (((Lp + 3) / 4) + 3) / 4 : 0;
    g.sh = Lp > 0 ? (4 - (i0 & 3)) & 3 : 0;
    int need = std::max(g.sh + m->L, g.sh + i0 + 16 * g.NC);
    g.Ls = (need + 3) & ~3;
    if (((g.Ls >> 2) & 1) == 0) g.Ls += 4;   // odd number of dwords per row: strided LDS reads of state rows hit distinct banks
}

// A population of states as the expert kernels read it: rows in state layout (CNN, chain kernels) and the transposed
// window letters (Potts kernel; potts.h "T4").
struct States {
    const uint8_t* rows;
    const uint32_t* T;
    int n_pad;
};
static int state_rows_to_t4(const ppde_model* m, const uint8_t* rows, uint32_t* T, int n, int n_pad, hipStream_t s) {
    if (m->g.Lp <= 0 || n <= 0) return PPDE_OK;
    const int tot = n * 16 * m->g.NC;
    hipLaunchKernelGGL(k_state_to_t4, dim3((tot + 255) / 256), dim3(256), 0, s, rows, T, n, n_pad, m->g);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

static int upload_wt(ppde_model* m) {
    if (m->d_wt) { uint8_t* old = m->d_wt; m->d_wt = nullptr; HIPCHK(hipFree(old)); }   // (never left dangling if what follows fails)
    std::vector<uint8_t> row(m->g.Ls, 0);
    for (int l = 0; l < m->L; ++l) row[m->g.sh + l] = m->h_wt[l];
    HIPCHK(dalloc(&m->d_wt, (size_t)m->g.Ls));
    HIPCHK(hipMemcpy(m->d_wt, row.data(), row.size(), hipMemcpyHostToDevice));
    if (m->d_wtT) { hipFree(m->d_wtT); m->d_wtT = nullptr; }
    if (m->g.Lp > 0) {
        const size_t words = potts_t4_words(m->g.NC, potts_t4_pad(1));
        HIPCHK(dalloc(&m->d_wtT, words));
        HIPCHK(hipMemset(m->d_wtT, 0, words * sizeof(uint32_t)));
        int rc = state_rows_to_t4(m, m->d_wt, m->d_wtT, 1, potts_t4_pad(1), 0);
        if (rc) return rc;
        HIPCHK(hipDeviceSynchronize());
    }
    return PPDE_OK;
}

static void free_scratch(ppde_model* m) {
    hipFree(m->s_state); hipFree(m->s_stateT); hipFree(m->s_grad); hipFree(m->s_epart); hipFree(m->s_gradC); hipFree(m->s_fitC);
    m->s_state = nullptr; m->s_stateT = nullptr; m->s_grad = m->s_epart = m->s_gradC = m->s_fitC = nullptr;
    m->scratch_n = 0;
}

// Launch the experts on states in state layout. Outputs go to slot buffers laid out as in PasArgs.
struct EvalTargets {
    float* grad;      // [slots][n][N]
    float* epart;     // [slots][n][Lp]
    float* gradC;     // [slots][nets][n][N]
    float* fitC;      // [slots][nets][n]
    int slot;
    unsigned long long* dbg = nullptr;
    // chunk maxima / arg-max rows / ReLU gate bits of the long-sequence CNN path. They belong to whoever owns the
    // slot buffers (one set per ppde_chains, one for the stateless API), never to the model: a captured hipGraph
    // has these pointers baked into its kernel arguments, and two owners run on different streams.
    float* cmax = nullptr;
    int* carg = nullptr;
    uint32_t* cgate = nullptr;
    int cnn_cap = 0;          // chains the chunk scratch is sized for
    // transformer expert: gradient rows [slots][n][N], scores [slots][n], and the owner's activation workspace
    float* gradT = nullptr;
    float* tfE = nullptr;
    TfWork* tfw = nullptr;
};

// chain groups (of 64) per Potts workgroup. Measured with this round's kernel (scripts/tune_potts.py, us per launch, wild-type /
// random states): 128 chains: 1 group 5.08, 2 groups 4.66, 4 groups 5.63; 512 chains: 8.7 / 7.8 / 9.0; 1024: 13.0 / 12.1 / 13.8;
// 2048: 21.8 / 20.3 / 22.9 (random states +1 to +3 us). Beyond ~512 chains the kernel is bound by the gather itself, not by
// the stream: 80 rows x 16 B per chain and tile are 524 MB of LDS reads per launch at 1024 chains (6.7 us at the chip's
// 128 B/clk/CU) next to 5 vector instructions per row (8.4 us); walking several chain blocks per workgroup on one resident
// slab (one stream of the couplings per tile instead of one per block) was built and measured equal (13.8 us at 1024).
static int potts_ng_for(int n) { return n <= 64 ? 1 : 2; }


// When set, EVERY kernel of the timed iterations (chain kernels and Potts launches) is launched through hipExtLaunchKernelGGL
// with a STOP event from this pool bound to its dispatch: the kernel's own end timestamp as the command processor records it, the
// source rocprofv3's kernel trace reads, with no extra packet on the stream (an hipEventRecord pair around a launch adds two
// barrier packets and ~2 us to what it measures; a start event of hipExtLaunchKernelGGL is a marker packet of its own). A Potts
// launch is then timed from its predecessor's end to its own end, which is how rocprofv3's per-kernel table accounts a
// dependent kernel of a stream (its interval starts where the predecessor's ends).
struct EventPool {
    std::vector<hipEvent_t> ev;
    std::vector<char> is_potts;
    size_t used = 0;
    bool exhausted = false;      // a launch went out untimed: the intervals are no longer predecessor -> successor
    ~EventPool() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    hipEvent_t next(bool potts) {
        if (used >= ev.size()) { exhausted = true; return nullptr; }
        is_potts[used] = potts ? 1 : 0;
        return ev[used++];
    }
};
static thread_local EventPool* g_potts_events = nullptr;

// One launch form for every expert and chain kernel: plain, or with a stop event bound to the dispatch (in-situ timing).
template <typename... P>
static void launch_kernel(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t stop, const P&... a) {
    if (stop) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, s, nullptr, stop, 0, a...);
    else hipLaunchKernelGGL(k, grid, block, lds, s, a...);
}
// A run-time int as a compile-time one: f(std::integral_constant<int, V>{}) for the V among Vs that equals v; false if none does.
// (Kernels come out in the library in the order the source first names them. The deduced return type has this helper instantiated
// where it is called, and the left fold instantiates f for Vs from first to last: source order here too.)
template <int... Vs, typename F>
static auto with_int(int v, F&& f) {
    return (... || (v == Vs && (f(std::integral_constant<int, Vs>{}), true)));
}

static PottsArgs potts_args(const ppde_model* m, const States& st, int n, const EvalTargets& t, int b_off, int n_sub) {
    PottsArgs a{};
    a.b_off = b_off; a.n_sub = n_sub; a.dbg = t.dbg;
    a.Jt = m->d_Jt; a.h = m->d_h; a.idxT = st.T; a.n_pad = st.n_pad; a.grad = t.grad; a.epart = t.epart;
    a.slot = t.slot; a.n = n;
    a.g = m->g;
    return a;
}

static int launch_potts(const ppde_model* m, const States& st, int n, const EvalTargets& t, hipStream_t s,
                        int b_off = 0, int n_sub = -1) {
    if (n_sub < 0) n_sub = n;
    hipEvent_t ev1 = g_potts_events ? g_potts_events->next(true) : nullptr;
    ARGCHK(st.T && st.n_pad >= n + 256, "the states have no transposed copy for the Potts kernel");
    const PottsArgs a = potts_args(m, st, n, t, b_off, n_sub);
    int NG = potts_ng_for(n_sub);
    static const int ng_override = env_int("PPDE_POTTS_NG", 0);   // tuning knob
    if (ng_override == 1 || ng_override == 2 || ng_override == 4) NG = ng_override;
    static const int ring_override = env_int("PPDE_POTTS_RING", -1);   // tuning knob
    const bool ring = ring_override >= 0 ? ring_override != 0 : m->g.NC > 8;   // long windows stream through a ring
    const int tiles = m->g.Lp * 5;
    // Every window of up to 256 residues (chunk counts 1..16) has an instantiation with its chunk count as a compile-time
    // constant (potts.h NCC): trip counts, DMA piece counts and counted waits are immediates there. Resident slab 5.12 ->
    // 4.96 us at PABP size, ring 17.7 -> 16.0 us at GFP size. PPDE_POTTS_SPEC=0: the general kernels (run-time chunk count).
    static const bool nc_spec = env_int("PPDE_POTTS_SPEC", 1) != 0;   // tuning knob
    if (ring) NG = std::min(NG, 2);
    const size_t lds = ring ? potts_ring_lds_bytes() : potts_lds_bytes(m->g.NC, NG);
    const int nby = (n_sub + NG * 64 - 1) / (NG * 64);
    auto go = [&](auto k) { launch_kernel(k, dim3(tiles * nby), dim3(256), lds, s, ev1, a, nby); };
    if (ring) {
        ARGCHK(m->g.NC <= 32, "Potts window longer than 512 residues");
        const bool g4 = potts_groups(m->g.NC) <= 4;             // letters of <= 4 chunk groups per wave: 5 workgroups per CU
        const bool pinned = nc_spec && g4 && with_int<9, 10, 11, 12, 13, 14, 15, 16>(m->g.NC, [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            go(NG == 1 ? potts_energy_grad_kernel<1, true, 4, NC> : potts_energy_grad_kernel<2, true, 4, NC>);
        });
        if (pinned) { }
        else if (NG == 1 && g4) go(potts_energy_grad_kernel<1, true, 4>);
        else if (NG == 1) go(potts_energy_grad_kernel<1, true, 8>);
        else if (g4) go(potts_energy_grad_kernel<2, true, 4>);
        else go(potts_energy_grad_kernel<2, true, 8>);
    } else {
        ARGCHK(m->g.NC <= 8, "Potts window too long for the resident-slab kernel (the ring variant takes it)");
        const bool pinned = nc_spec && NG <= 2 && with_int<1, 2, 3, 4, 5, 6, 7, 8>(m->g.NC, [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            go(NG == 1 ? potts_energy_grad_kernel<1, false, 2, NC> : potts_energy_grad_kernel<2, false, 2, NC>);
        });
        if (pinned) { }
        else if (NG == 1) go(potts_energy_grad_kernel<1>);
        else if (NG == 2) go(potts_energy_grad_kernel<2>);
        else go(potts_energy_grad_kernel<4>);
    }
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// Both dense contractions of the CNN on the bf16 matrix pipe (split-precision, cnn.h bf_strips): the default.
// PPDE_CNN_BF16=0 keeps the exact-fp32 MFMA kernels (v_mfma_f32_16x16x4_f32).
static bool cnn_bf16() {
    static const bool on = env_int("PPDE_CNN_BF16", 1) != 0;   // tuning knob
    return on;
}
static size_t cnn_single_lds(const ppde_model* m) {
    return cnn_bf16() ? cnn_bf_lds_bytes(m->T, m->CP, m->FP, m->J, m->L) : cnn_lds_bytes(m->T, m->CP, m->FP, m->J, m->L);
}
// launch form of a supervised expert of this (padded) shape: single launch, or the forward / backward chunk kernels
static bool cnn_single_launch_shape(int T, int CP, int FP, int J, int L) {
    static const int chunked_override = env_int("PPDE_CNN_CHUNKED", -1);   // tuning knob
    if (chunked_override == 1) return false;
    const size_t lds = cnn_bf16() ? cnn_bf_lds_bytes(T, CP, FP, J, L) : cnn_lds_bytes(T, CP, FP, J, L);
    if (cnn_rows(T) > 16 * CNN_MAX_RT || lds > 160 * 1024 || FP > 512) return false;   // (cnn_body keeps two features per thread)
    // Where only ONE workgroup of the single-launch kernel fits a CU (L >= 100), the chunked path (two to four
    // workgroups per CU, balanced grids) is faster: UBE4B, L = 104: 166 us/step against 214 (180 with an 8-wave
    // variant of the single-launch kernel that was built and dropped again). PABP (two per CU): 108 vs 136.
    return 2 * lds <= 160 * 1024 || chunked_override == 0;
}
static bool cnn_single_launch(const ppde_model* m) { return cnn_single_launch_shape(m->T, m->CP, m->FP, m->J, m->L); }

// The chunk kernels keep 64 rows of ALL padded channels in LDS (forward: the split h1 image; backward: the routed gradient's, 12
// bytes per padded feature beside it): what bounds the width of a network that does not fit the single-launch kernel.
static size_t cnn_chunk_lds(int CP, int FP, int J) {
    const bool bf = cnn_bf16();
    const size_t lds_f = bf ? cnn_bf_fwd_chunk_lds(CP, FP) : cnn_fwd_chunk_lds(CP);
    const size_t lds_b = bf ? cnn_bf_bwd_chunk_lds(CP, FP, J) : cnn_bwd_chunk_lds(CP, FP, J);
    return std::max(lds_f, lds_b);
}
// "" if the chunk kernels serve this width, else the refusal (the bound in channels at this embedding width)
static std::string cnn_chunk_refusal(int C, int CP, int F, int FP, int J) {
    // the backward window's route bitmap (one bit per row and padded feature) lies in the storage the routed gradient takes after
    // it (k_cnn_bwd_chunk: sB = sD): it must fit there, or it runs into the gate bits behind it. (The exact-fp32 layout is held to
    // its own routed-gradient rows: cautious there, where what lies behind is written only after the routing.)
    const size_t rows_b = cnn_bf16() ? CNN_BCH_RT * 16 : CNN_BCH_RT_F32 * 16, bitmap = rows_b * ((FP + 31) / 32) * 4;
    const size_t region = cnn_bf16() ? std::max((size_t)CNN_BCH_RT * BFT * (CP / 32) * 1024, rows_b * J * 4) : rows_b * cnn_astride(CP) * 4;
    if (bitmap > region)
        return "supervised expert: F = " + std::to_string(F) + " features are too many for the chunked CNN kernels at C = " + std::to_string(C) +
               " channels: F (padded to 16) <= 32 * max(C padded to 32, 20 * taps), here " + std::to_string(region / (rows_b / 8));
    if (cnn_chunk_lds(CP, FP, J) <= 160 * 1024) return "";
    int cp_max = 0;
    for (int cp = 32; cp < CP; cp += 32) if (cnn_chunk_lds(cp, FP, J) <= 160 * 1024) cp_max = cp;
    return "supervised expert too wide for the chunked CNN kernels: C = " + std::to_string(C) + " channels (padded to " +
           std::to_string(CP) + ") with F = " + std::to_string(F) + " features need more than 160 KiB of LDS; at this F at most " +
           std::to_string(cp_max) + " channels (reference-shaped networks, C = L and F = 2L: L <= 544)";
}

// Output rows of the CNN expert per chain. The single-launch kernel cuts the LAST network's features into two workgroups:
// chains x networks workgroups on 256 CUs at two per CU left half of the CUs with one workgroup (32 us) and half with
// two (45 us) at 128 chains x 3 networks; with 2 whole + 2 half units per chain every CU pairs a whole unit with a half
// one. The cut does not depend on the batch (a chain's numbers never depend on the batch it sits in).
static int cnn_parts(const ppde_model* m) {
    static const bool split = env_int("PPDE_CNN_SPLIT", 1) != 0;   // tuning knob
    if (!m->has_cnn) return std::max(m->n_nets, 1);
    return (split && cnn_single_launch(m) && m->n_nets <= 3 && m->FP >= 32) ? m->n_nets + 1 : m->n_nets;
}

// row tiles of a forward chunk of the long-sequence CNN path (cnn.h: 4, or 3 for the split-precision kernels beyond 128 channels)
static int cnn_fwd_rt(const ppde_model* m) { return cnn_bf16() ? cnn_bf_fwd_rt(m->CP) : CNN_FCH_RT; }
static size_t cnn_chunk_max_count(const ppde_model* m, int n) { return (size_t)m->n_nets * n * cnn_fwd_chunks(m->T, cnn_fwd_rt(m)) * m->FP; }
static size_t cnn_chunk_gate_count(const ppde_model* m, int n) {
    return (size_t)m->n_nets * n * cnn_fwd_chunks(m->T, cnn_fwd_rt(m)) * cnn_fwd_rt(m) * 16 * ((m->CP + 31) / 32);
}
// chunk scratch of the STATELESS API only (ppde_energy_grad); every ppde_chains owns its own (ppde_chains_create)
static int ensure_cnn_scratch(ppde_model* m, int n) {
    if (cnn_single_launch(m) || n <= m->cnn_scratch_n) return PPDE_OK;
    hipFree(m->cnn_cmax); hipFree(m->cnn_carg); hipFree(m->cnn_cgate);
    m->cnn_cmax = nullptr; m->cnn_carg = nullptr; m->cnn_cgate = nullptr; m->cnn_scratch_n = 0;
    HIPCHK(dalloc(&m->cnn_cmax, cnn_chunk_max_count(m, n)));
    HIPCHK(dalloc(&m->cnn_carg, cnn_chunk_max_count(m, n)));
    HIPCHK(dalloc(&m->cnn_cgate, cnn_chunk_gate_count(m, n)));
    m->cnn_scratch_n = n;
    return PPDE_OK;
}

// gsc = 2^-ceil(log2 |scale|) and its reciprocal: |scale| * gsc <= 1, so the static bound behind CnnNet.sc_g (taken at |scale| = 1)
// holds for the routed gradient of this launch (cnn.h, two-term split)
static void cnn_grad_scale(float scale, float* gsc, float* gun) {
    const float a = fabsf(scale);
    int e = 0;
    if (a > 0.f && a < 3.0e38f) {
        const float mnt = frexpf(a, &e);                              // a = mnt 2^e, mnt in [0.5, 1)
        if (mnt == 0.5f) --e;                                         // (a power of two: a * 2^-(e-1) = 1)
    }
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    *gsc = ldexpf(1.f, -e);
    *gun = ldexpf(1.f, e);
}

static CnnArgs cnn_args(const ppde_model* m, const States& st, int n, const EvalTargets& t, int want_grad, float scale, int b_off) {
    CnnArgs a{};
    a.b_off = b_off; a.dbg = t.dbg;
    for (int k = 0; k < m->n_nets; ++k) a.net[k] = m->nets[k];
    a.n_nets = m->n_nets; a.n_parts = cnn_parts(m); a.C = m->C; a.CP = m->CP; a.K = m->K; a.KT = m->KT; a.F = m->F; a.FP = m->FP; a.T = m->T; a.J = m->J; a.JP = m->JP;
    a.idx = st.rows; a.gradC = t.gradC; a.fitC = t.fitC;
    a.slot = t.slot; a.n = n; a.want_grad = want_grad; a.scale = scale;
    cnn_grad_scale(scale, &a.gsc, &a.gun);
    a.g = m->g;
    return a;
}

// The network shapes that have shape-pinned instantiations (PPDE_CNN_SPEC=0: the general kernels everywhere). The host selects
// a pinned kernel only for exactly its shape: every trip count in it is a compile-time constant.
static bool cnn_shape_spec() {
    static const bool on = env_int("PPDE_CNN_SPEC", 1) != 0;   // tuning knob
    return on;
}
static bool cnn_five_taps(const ppde_model* m) { return m->KT == 5 && m->K == 5 && m->J == 100 && m->JP == 112; }
// backward chunks (cnn.h CnnChunkShape): 1 = the UBE4B networks, 2 = the GFP networks
static bool cnn_is_ube4b_shape(const ppde_model* m) { return cnn_five_taps(m) && m->T == 100 && m->CP == 128 && m->F == 208 && m->FP == 208; }
static bool cnn_is_gfp_shape(const ppde_model* m) { return cnn_five_taps(m) && m->T == 233 && m->CP == 256 && m->F == 474 && m->FP == 480; }
// the fused launch: the PABP_YEAST networks (three in four output rows) beside a five-chunk Potts window, two chain groups
static bool experts_is_pabp_shape(const ppde_model* m, int NG, int n_parts) {
    return NG == 2 && m->L == 96 && m->g.NC == 5 && m->C == 96 && m->CP == 96 && m->K == 5 && m->F == 192 && m->FP == 192 && m->T == 92 &&
           m->J == 100 && m->JP == 112 && m->n_nets == 3 && n_parts == 4;
}

static int launch_cnn(const ppde_model* m, const States& st, int n, const EvalTargets& t, int want_grad,
                      float scale, hipStream_t s, int b_off = 0, int n_sub = -1) {
    if (n_sub < 0) n_sub = n;
    const CnnArgs a = cnn_args(m, st, n, t, want_grad, scale, b_off);
    const bool bf = cnn_bf16(), k5 = m->KT == 5;
    if (!cnn_single_launch(m)) {
        // long sequences: forward chunks, then merge + backward chunks
        ARGCHK(t.cmax && t.carg && t.cgate && t.cnn_cap >= n, "CNN chunk scratch not allocated for this batch size");
        const int frt = cnn_fwd_rt(m);
        const size_t lds_f = bf ? cnn_bf_fwd_chunk_lds(m->CP, m->FP) : cnn_fwd_chunk_lds(m->CP);
        const size_t lds_b = bf ? cnn_bf_bwd_chunk_lds(m->CP, m->FP, m->J) : cnn_bwd_chunk_lds(m->CP, m->FP, m->J);
        // (ppde_model_set_cnn refuses such a shape; this is the backstop in front of the launch)
        ARGCHK(lds_f <= 160 * 1024 && lds_b <= 160 * 1024, cnn_chunk_refusal(m->C, m->CP, m->F, m->FP, m->J));
        CnnChunkArgs ca{a, t.cmax, t.carg, t.cgate, cnn_fwd_chunks(m->T, frt), frt * 16};
        const dim3 gf(n_sub, m->n_nets, ca.NCH), gb(n_sub, m->n_nets, want_grad ? cnn_bwd_chunks(m->L, m->KT, bf) : 1);
        // the two long real proteins have instantiations with their network shape pinned (cnn.h CnnChunkShape). Only the BACKWARD
        // chunks: with the trip counts known the forward chunk kernel is measured slower -- UBE4B 32.1 -> 47.3 us, GFP 244 -> 674 us
        // per launch; the backward gains: 33.9 -> 30.1 and 125.8 -> 116.3.
        const int shape = !cnn_shape_spec() ? 0 : cnn_is_ube4b_shape(m) ? 1 : cnn_is_gfp_shape(m) ? 2 : 0;
        // Split-precision chunks (16-bit matrix pipe): forward chunks and backward windows of 64 rows.
        // Networks of more than 128 channels (GFP: two chunk workgroups per CU by LDS) run the chunk kernels with 512 threads:
        // four waves per SIMD hide what a block's instruction stream costs better than the second A register set of the
        // 256-thread form (GFP + CNN 505 -> 446 us per step, A/B on one box); up to 128 channels three 256-thread workgroups
        // share a CU and 512 threads lose (UBE4B 104.2 -> 106.6). PPDE_CNN_CHUNK_512=0 keeps 256 threads everywhere. Same bits.
        static const bool allow512 = env_int("PPDE_CNN_CHUNK_512", 1) != 0;
        const bool wide = bf && allow512 && m->CP > 128;
        void (*fwd)(CnnChunkArgs);
        void (*bwd)(CnnChunkArgs);
        if (wide) {
            fwd = k5 ? k_cnn_fwd_chunk<5, 0, CNN_WIDE_FRT, true, 512> : k_cnn_fwd_chunk<CNN_MAX_K, 0, CNN_WIDE_FRT, true, 512>;
            bwd = k5 ? (shape == 2 ? k_cnn_bwd_chunk<5, 2, true, 512> : k_cnn_bwd_chunk<5, 0, true, 512>) : k_cnn_bwd_chunk<CNN_MAX_K, 0, true, 512>;
        } else if (bf) {
            fwd = k5 ? (frt == 4 ? k_cnn_fwd_chunk<5, 0, 4, true> : k_cnn_fwd_chunk<5, 0, 3, true>)
                     : (frt == 4 ? k_cnn_fwd_chunk<CNN_MAX_K, 0, 4, true> : k_cnn_fwd_chunk<CNN_MAX_K, 0, 3, true>);
            bwd = shape ? (shape == 1 ? k_cnn_bwd_chunk<5, 1, true> : k_cnn_bwd_chunk<5, 2, true>)
                        : k5 ? k_cnn_bwd_chunk<5, 0, true> : k_cnn_bwd_chunk<CNN_MAX_K, 0, true>;
        } else if (k5) {
            fwd = k_cnn_fwd_chunk<5>;
            bwd = shape ? (shape == 1 ? k_cnn_bwd_chunk<5, 1> : k_cnn_bwd_chunk<5, 2>) : k_cnn_bwd_chunk<5>;
        } else {
            fwd = k_cnn_fwd_chunk<CNN_MAX_K>;
            bwd = k_cnn_bwd_chunk<CNN_MAX_K>;
        }
        const dim3 block(wide ? 512 : 256);
        launch_kernel(fwd, gf, block, lds_f, s, nullptr, ca);
        launch_kernel(bwd, gb, block, lds_b, s, nullptr, ca);
        HIPCHK(hipGetLastError());
        return PPDE_OK;
    }
    const size_t lds = cnn_single_lds(m);
    const dim3 grid(n_sub, a.n_parts);
    const int rt = cnn_rows(m->T) / 16;
    with_int<1, 2, 3, 4, 5, 6, 7, 8>(rt >= 1 && rt <= 7 ? rt : 8, [&](auto rtc) {
        constexpr int RT = decltype(rtc)::value;
        launch_kernel(bf ? (k5 ? k_cnn<RT, 5, CNN_NT, true> : k_cnn<RT, CNN_MAX_K, CNN_NT, true>) : (k5 ? k_cnn<RT, 5> : k_cnn<RT, CNN_MAX_K>),
                      grid, dim3(CNN_NT), lds, s, nullptr, a);
    });
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// Both experts in ONE launch. The CNN grid (chains x networks workgroups, two per CU by LDS) comes first in block
// order; once it exceeds the CU count, every further workgroup shares a CU with an earlier one and the CUs beyond
// (grid - CUs) hold a single one with half of their LDS and wave slots idle for the whole launch (measured: 32 us
// alone vs 37 / 45 us for a pair). The Potts tiles come last in block order, so they are placed into exactly those
// free slots and finish long before the paired CNN workgroups: the Potts evaluation costs no time of its own and
// one launch boundary disappears. (Running the two kernels on two streams of a captured graph was measured 24 us
// per iteration SLOWER: fork/join inside a hipGraph is expensive.)
struct ExpertsArgs {
    CnnArgs c;
    PottsArgs p;
    int cnn_bx, cnn_ni;        // CNN workgroups = cnn_bx (chains) x cnn_ni (networks), first in block order
    int potts_items, potts_nby;   // then potts_items = tiles x potts_nby (chain blocks) Potts workgroups
};
// PABP: the CNN's shape pinned to the PABP_YEAST networks' (L = 96: 96 channels, 192 features, 5 taps, three networks in four
// output rows, gradients wanted), so that every trip count of cnn_body is a compile-time constant (as pin_config in pas.h)
// Block order of the fused launch: the two HALF units of every chain first, the whole units second -- a CU's first workgroup is
// the older one and wins the issue arbitration (priority, then age), so the unit with less work finishes early and the whole unit
// has the CU to itself for its remainder (k_experts 28.7 -> 28.1 us, A/B on one box; with the whole units first the half unit
// crawls beside them and finishes last). The Potts tiles in front measured slower, and no s_setprio experiment was kept
// (profiles/r05_experiments.md). Outputs do not depend on the order.
// Waves per SIMD the shape-pinned split-precision instantiation is compiled for. (Six -- 80 registers, three workgroups per CU --
// returned wrong gradients a few times in thousands of evaluations: DESIGN.md.)
constexpr int PPDE_EXPERTS_WAVES = 4;
template <int RT, int NG, bool PABP = false, bool BF = false>
__global__ __launch_bounds__(CNN_NT, (PABP && BF) ? PPDE_EXPERTS_WAVES : (RT <= 6 ? 4 : 2)) void k_experts(ExpertsArgs a) {
    warm_kernargs<sizeof(ExpertsArgs)>();

    extern __shared__ float4 smem_experts[];
    const int n_cnn = a.cnn_bx * a.cnn_ni;
    const int w = blockIdx.x;
    if (w < n_cnn) {
        const int nw = w / a.cnn_bx;
        const int ni = a.cnn_ni == 4 ? ((nw + 2) & 3) : nw;       // (the half units first in block order)
        if constexpr (BF) cnn_body_bf<RT, 5, CNN_NT, PABP>(a.c, w - nw * a.cnn_bx, ni, a.cnn_bx, a.cnn_ni, (unsigned char*)smem_experts);
        else cnn_body<RT, 5, CNN_NT, PABP>(a.c, w - nw * a.cnn_bx, ni, a.cnn_bx, a.cnn_ni, (unsigned char*)smem_experts);
    } else {
        if (threadIdx.x >= 256) return;          // a Potts tile is the work of four waves (the barrier counts live waves only)
        const int v = xcd_contiguous(w - n_cnn, a.potts_items);
        potts_body<NG, false, 2, PABP ? 5 : 0>(a.p, v / a.potts_nby, v % a.potts_nby, smem_experts);
    }
}

static int launch_experts_fused(const ppde_model* m, const States& st, int n, const EvalTargets& t, float scale,
                                hipStream_t s, int b_off, int n_sub, bool* done) {
    *done = false;
    static const bool enabled = env_int("PPDE_FUSE_EXPERTS", 1) != 0;
    const int NG = potts_ng_for(n_sub);
    if (!enabled || !cnn_single_launch(m) || m->KT != 5 || NG > 2 || g_potts_events) return PPDE_OK;
    const size_t lds_c = cnn_single_lds(m), lds_p = potts_lds_bytes(m->g.NC, NG);
    const bool bf = cnn_bf16();
    if (lds_p > lds_c || 2 * lds_c > 160 * 1024 || m->g.NC > 8) return PPDE_OK;   // (needs the free second slot)
    ExpertsArgs a{};
    a.c = cnn_args(m, st, n, t, 1, scale, b_off);
    a.p = potts_args(m, st, n, t, b_off, n_sub);
    a.p.dbg_wg_base = 1024;
    a.cnn_bx = n_sub; a.cnn_ni = a.c.n_parts;
    const int CPB = NG * 64;
    a.potts_nby = (n_sub + CPB - 1) / CPB;
    a.potts_items = m->g.Lp * 5 * a.potts_nby;
    const dim3 grid(a.cnn_bx * a.cnn_ni + a.potts_items);
    auto go = [&](auto k) { launch_kernel(k, grid, dim3(CNN_NT), lds_c, s, nullptr, a); };
    if (cnn_shape_spec() && experts_is_pabp_shape(m, NG, a.c.n_parts)) {
        go(bf ? k_experts<6, 2, true, true> : k_experts<6, 2, true>);
    } else {
        const int rt = cnn_rows(m->T) / 16;
        with_int<1, 2, 3, 4, 5, 6, 7, 8>(rt >= 1 && rt <= 7 ? rt : 8, [&](auto rtc) {
            constexpr int RT = decltype(rtc)::value;
            go(bf ? (NG == 1 ? k_experts<RT, 1, false, true> : k_experts<RT, 2, false, true>) : (NG == 1 ? k_experts<RT, 1> : k_experts<RT, 2>));
        });
    }
    HIPCHK(hipGetLastError());
    *done = true;
    return PPDE_OK;
}

// Experts whose gradient is part of grad_x for an energy `which` (bits 0-2 experts, bit 3 = PPDE_WHICH_FULL_GRAD).
// Reference: the potts branch differentiates e = dH + lamda * fit w.r.t. x (energy.py:105-108); the transformer /
// potts+transformer branch computes fit from x but differentiates w.r.t. the SLICE x_batch (energy.py:115, :125), so
// lamda * d fit/dx never reaches grad_x there: the supervised expert shapes the energy and the accept step, not the
// proposal. Bit 3 opts into the full gradient instead.
static int grad_sources(int which) {
    const int w = which & 7;
    return ((w & 4) && !(which & PPDE_WHICH_FULL_GRAD)) ? (w & ~2) : w;
}

static int eval_experts(const ppde_model* m, int which, const States& states, int n, const EvalTargets& t,
                        int want_grad, hipStream_t s, int b_off = 0, int n_sub = -1) {
    const int gw = grad_sources(which);
    which &= 7;
    const int cnn_grad = want_grad && (gw & 2);       // (no CNN backward where its gradient is not used)
    if ((which & 3) == 3 && cnn_grad && m->has_potts && m->has_cnn) {   // (Potts + CNN in one launch; the transformer follows)
        bool done = false;
        int rc = launch_experts_fused(m, states, n, t, m->lamda / (float)m->n_nets, s, b_off, n_sub < 0 ? n : n_sub, &done);
        if (rc) return rc;
        if (done) which &= ~3;
    }
    if (which & 1) {
        ARGCHK(m->has_potts, "the energy uses the Potts expert but ppde_model_set_potts was not called");
        int rc = launch_potts(m, states, n, t, s, b_off, n_sub);
        if (rc) return rc;
    }
    if (which & 2) {
        ARGCHK(m->has_cnn, "the energy uses the supervised expert but ppde_model_set_cnn was not called");
        float scale = (which == 2 ? 1.0f : m->lamda) / (float)m->n_nets;
        int rc = launch_cnn(m, states, n, t, cnn_grad, scale, s, b_off, n_sub);
        if (rc) return rc;
    }
    if (which & 4) {
        ARGCHK(m->tf, "the energy uses the transformer expert but ppde_model_set_transformer was not called");
        ARGCHK(t.tfw && t.tfE && (t.gradT || !want_grad), "no transformer workspace for this evaluation");
        const int ns = n_sub < 0 ? n : n_sub;
        int rc = tf_eval(m->tf, t.tfw, states.rows + (size_t)b_off * m->g.Ls, m->g.Ls, m->g.sh, ns, t.tfE + (size_t)t.slot * n + b_off,
                         want_grad ? t.gradT + ((size_t)t.slot * n + b_off) * m->g.N : nullptr, s);
        if (rc) return rc;
    }
    return PPDE_OK;
}

static PasArgs base_pas_args(const ppde_model* m, int which, int n) {
    PasArgs a{};
    a.g = m->g; a.n = n; a.wt = m->d_wt; a.wt_H = m->wt_H; a.lamda = m->lamda; a.which = which & 7; a.gwhich = grad_sources(which);
    a.n_nets = m->n_nets; a.n_parts = cnn_parts(m);
    a.tf_wt = m->tf ? m->tf->wt_score : 0.f;
    return a;
}

// --------------------------------------------------------------------------------------------
extern "C" {

int ppde_abi_version(void) { return PPDE_ABI_VERSION; }
const char* ppde_last_error(void) { return g_err.c_str(); }

int ppde_device_count(void) {
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    return n;
}

int ppde_model_create(ppde_model** out, int device, int L, const uint8_t* wt_idx) {
    ARGCHK(out && wt_idx, "null argument");
    ARGCHK(L >= 5 && L <= 4096, "sequence length out of range");
    for (int l = 0; l < L; ++l) ARGCHK(wt_idx[l] < PPDE_A, "wild-type residue index out of range");
    HIPCHK(hipSetDevice(device));
    ppde_model* m = new ppde_model();
    m->device = device;
    m->L = L;
    m->h_wt.assign(wt_idx, wt_idx + L);
    set_geom(m, 0, 0);
    int rc = upload_wt(m);
    if (rc) { delete m; return rc; }
    *out = m;
    return PPDE_OK;
}

int ppde_model_destroy(ppde_model* m) {
    if (!m) return PPDE_OK;
    hipSetDevice(m->device);
    free_scratch(m);
    hipFree(m->s_flag);
    hipFree(m->d_wt); hipFree(m->d_wtT); hipFree(m->d_Jt); hipFree(m->d_h); hipFree(m->cnn_cmax); hipFree(m->cnn_carg); hipFree(m->cnn_cgate);
    for (void* p : m->cnn_allocs) hipFree(p);
    hipFree(m->s_gradT); hipFree(m->s_tfE);
    delete m->s_tfw;
    delete m->tf;
    delete m;
    return PPDE_OK;
}

int ppde_model_set_lamda(ppde_model* m, float lamda) {
    ARGCHK(m, "null model");
    m->lamda = lamda;
    return PPDE_OK;
}

int ppde_model_set_transformer(ppde_model* m, int n_layers, int dim, int heads, int ffn, const ppde_tf_weights* w) {
    ARGCHK(m && w, "null argument");
    ARGCHK(n_layers >= 1 && n_layers <= 64, "1..64 transformer layers");
    ARGCHK(heads >= 1 && (dim == heads * 24 || dim == heads * 32 || dim == heads * 64),
           "the attention kernels are written for head widths 24, 32 and 64 (ESM-2 35M: 480 / 20, 150M: 640 / 20, 650M: 1280 / 20)");
    ARGCHK(dim % 8 == 0 && ffn % 128 == 0 && dim <= TF_LN_MAXD, "dim must be a multiple of 8 (<= 1536), ffn a multiple of 128");
    ARGCHK(m->L <= TF_TP_MAX, "the transformer expert handles sequences of up to 256 residues");
    // every parameter finite in fp32, every matrix entry finite at the fp16 value the device multiplies (|w| < 65520):
    // checked before anything is touched, so that a refusal leaves the expert that was there
    {
        int rc = PPDE_OK;
        auto finite = [&](const char* name, int layer, const float* v, size_t count, bool matrix) {
            if (rc != PPDE_OK) return;
            if (!v) { rc = fail(PPDE_ERR_INVALID, std::string("null transformer parameter ") + name); return; }
            for (size_t i = 0; i < count; ++i) {
                const bool ok = matrix ? std::isfinite((float)(half_t)v[i]) : std::isfinite(v[i]);
                if (ok) continue;
                rc = fail(PPDE_ERR_INVALID, std::string("transformer parameter ") + name + (layer >= 0 ? " of layer " + std::to_string(layer) : std::string())
                                                + ": entry " + std::to_string(i) + (std::isfinite(v[i]) ? " is beyond fp16's largest value 65504, the format the matrices are multiplied in"
                                                                                                        : " is not finite"));
                return;
            }
        };
        const size_t D = (size_t)dim, F = (size_t)ffn;
        finite("embed_tokens.weight", -1, w->embed, (size_t)TF_VOCAB * D, true);
        const float* const* per_layer[] = {w->q_w, w->q_b, w->k_w, w->k_b, w->v_w, w->v_b, w->o_w, w->o_b, w->ln1_w, w->ln1_b, w->ln2_w, w->ln2_b,
                                           w->fc1_w, w->fc1_b, w->fc2_w, w->fc2_b};
        for (auto p : per_layer) ARGCHK(p, "null per-layer transformer parameter array");
        for (int l = 0; l < n_layers; ++l) {
            finite("self_attn.q_proj.weight", l, w->q_w[l], D * D, true);   finite("self_attn.q_proj.bias", l, w->q_b[l], D, false);
            finite("self_attn.k_proj.weight", l, w->k_w[l], D * D, true);   finite("self_attn.k_proj.bias", l, w->k_b[l], D, false);
            finite("self_attn.v_proj.weight", l, w->v_w[l], D * D, true);   finite("self_attn.v_proj.bias", l, w->v_b[l], D, false);
            finite("self_attn.out_proj.weight", l, w->o_w[l], D * D, true); finite("self_attn.out_proj.bias", l, w->o_b[l], D, false);
            finite("self_attn_layer_norm.weight", l, w->ln1_w[l], D, false); finite("self_attn_layer_norm.bias", l, w->ln1_b[l], D, false);
            finite("final_layer_norm.weight", l, w->ln2_w[l], D, false);     finite("final_layer_norm.bias", l, w->ln2_b[l], D, false);
            finite("fc1.weight", l, w->fc1_w[l], F * D, true);               finite("fc1.bias", l, w->fc1_b[l], F, false);
            finite("fc2.weight", l, w->fc2_w[l], D * F, true);               finite("fc2.bias", l, w->fc2_b[l], D, false);
        }
        finite("emb_layer_norm_after.weight", -1, w->final_ln_w, D, false);  finite("emb_layer_norm_after.bias", -1, w->final_ln_b, D, false);
        finite("lm_head.dense.weight", -1, w->head_dense_w, D * D, true);    finite("lm_head.dense.bias", -1, w->head_dense_b, D, false);
        finite("lm_head.layer_norm.weight", -1, w->head_ln_w, D, false);     finite("lm_head.layer_norm.bias", -1, w->head_ln_b, D, false);
        finite("lm_head.bias", -1, w->head_bias, (size_t)TF_VOCAB, false);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(m->device));
    // the new expert is built completely, the wild type's score included, before the old one is let go
    TfModel* t = new TfModel();
    t->layers = n_layers; t->Dr = dim; t->D = (dim + 127) & ~127; t->H = heads; t->F = ffn; t->HD = dim / heads;
    int rc = tf_build_model(t, m->L, w);
    if (rc) { delete t; return rc; }
    // wild type's local score (nets.py:188) with the kernels that evaluate every other state
    {
        TfWork wk;
        DevBuf<float> sc;
        if ((rc = tf_alloc_work(t, &wk, 1)) == PPDE_OK && sc.alloc(1) != hipSuccess) rc = fail(PPDE_ERR_HIP, "allocation failed");
        if (rc == PPDE_OK) rc = tf_eval(t, &wk, m->d_wt, m->g.Ls, m->g.sh, 1, sc.p, nullptr, 0);
        if (rc == PPDE_OK && hipMemcpy(&t->wt_score, sc.p, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PPDE_ERR_HIP, "copy failed");
    }
    if (rc == PPDE_OK && !std::isfinite(t->wt_score))
        rc = fail(PPDE_ERR_NUMERIC, "the wild type's transformer score is not finite: an fp16 activation overflowed 65504 on these weights "
                                    "(see the supported range of the transformer expert in ppde_hip.h); every energy would be NaN");
    if (rc) { delete t; return rc; }
    delete m->tf; m->tf = t;
    delete m->s_tfw; m->s_tfw = nullptr;
    hipFree(m->s_gradT); hipFree(m->s_tfE); m->s_gradT = m->s_tfE = nullptr; m->s_tf_n = 0;
    return PPDE_OK;
}

// Timing hook for bench.py: the transformer's GEMM kernel (fc1 form: bias + GELU epilogue) on pseudo-random fp16
// operands of the given shape, `reps` launches between one HIP event pair on a stream of its own.
int ppde_transformer_time_gemm(int device, int M, int N, int K, int reps, int epilogue, float* avg_us) {
    ARGCHK(avg_us && reps >= 1 && M > 0 && N > 0 && K > 0, "bad argument");
    HIPCHK(hipSetDevice(device));
    // PPDE_TF_TIME_ROTATE=r (diagnostic): r sets of the [M][*] operands used in rotation, so that a launch finds its A rows and
    // second epilogue operand in HBM, as inside an evaluation, and not in the 256 MiB Infinity Cache the previous launch left them in
    static const int rot = std::min(std::max(env_int("PPDE_TF_TIME_ROTATE", 1), 1), 8);
    DevBuf<half_t> A[8], B, C[8], C2[8];
    DevBuf<float> bias;
    for (int r = 0; r < rot; ++r) {
        HIPCHK(A[r].alloc((size_t)M * K)); HIPCHK(C[r].alloc((size_t)M * N)); HIPCHK(C2[r].alloc((size_t)M * N));
    }
    HIPCHK(B.alloc((size_t)N * K)); HIPCHK(bias.alloc((size_t)N));
    HIPCHK(hipMemset(bias.p, 0, (size_t)N * sizeof(float)));
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct SG { hipStream_t s; ~SG() { hipStreamDestroy(s); } } sg{s};
    for (int r = 0; r < rot; ++r) {
        hipLaunchKernelGGL(tf_fill_random, dim3((unsigned)(((size_t)M * K + 255) / 256)), dim3(256), 0, s, A[r].p, (size_t)M * K, 1u + 16u * r);
        HIPCHK(hipMemsetAsync(C2[r].p, 0, (size_t)M * N * sizeof(half_t), s));
    }
    hipLaunchKernelGGL(tf_fill_random, dim3((unsigned)(((size_t)N * K + 255) / 256)), dim3(256), 0, s, B.p, (size_t)N * K, 2u);
    HIPCHK(hipGetLastError());
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
    int rc = PPDE_OK;
    auto one = [&](int i) {
        const half_t* a = A[i % rot].p;
        half_t *c = C[i % rot].p, *c2 = C2[i % rot].p;
        switch (epilogue) {
            case TF_EPI_PLAIN: return tf_gemm<TF_EPI_PLAIN>(s, a, B.p, c, M, N, K);
            case TF_EPI_BIAS: return tf_gemm<TF_EPI_BIAS>(s, a, B.p, c, M, N, K, bias.p);
            case TF_EPI_BIAS_RESID: return tf_gemm<TF_EPI_BIAS_RESID>(s, a, B.p, c, M, N, K, bias.p, c2);
            case TF_EPI_GELU_BWD: return tf_gemm<TF_EPI_GELU_BWD>(s, a, B.p, c, M, N, K, nullptr, c2);
            default: return tf_gemm<TF_EPI_BIAS_GELU>(s, a, B.p, c, M, N, K, bias.p, nullptr, c2);
        }
    };
    for (int i = 0; i < 3 && rc == PPDE_OK; ++i) rc = one(i);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev.a, s));
    for (int i = 0; i < reps && rc == PPDE_OK; ++i) rc = one(i + 3);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev.b, s));
    HIPCHK(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.f / reps;
    return PPDE_OK;
}

// The same kernel timed IN SITU: one stateless transformer evaluation (energy + gradient) of idx_dev [n, L] with a HIP event
// pair around every fc1 GEMM launch; mean event-to-event time and the number of launches timed.
int ppde_transformer_time_fc1_in_situ(ppde_model* m, const uint8_t* idx_dev, int n, float* avg_us, int* launches) {
    ARGCHK(m && m->tf && idx_dev && n >= 1 && avg_us && launches, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    DevBuf<float> e, fit, grad;
    HIPCHK(e.alloc((size_t)n)); HIPCHK(fit.alloc((size_t)n)); HIPCHK(grad.alloc((size_t)n * m->g.N));
    struct Guard { TfEventList l; ~Guard() { g_tf_fc1_events = nullptr; for (hipEvent_t x : l.ev) if (x) hipEventDestroy(x); } } g;
    g.l.ev.assign((size_t)2 * m->tf->layers, nullptr);
    for (auto& x : g.l.ev) HIPCHK(hipEventCreate(&x));
    int rc = ppde_energy_grad(m, idx_dev, n, 4, e.p, fit.p, grad.p, nullptr);   // warm (workspace, caches)
    if (rc) return rc;
    g_tf_fc1_events = &g.l;
    rc = ppde_energy_grad(m, idx_dev, n, 4, e.p, fit.p, grad.p, nullptr);
    g_tf_fc1_events = nullptr;
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    double tot = 0.0;
    int cnt = 0;
    for (size_t i = 0; i + 1 < g.l.used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g.l.ev[i], g.l.ev[i + 1]) == hipSuccess) { tot += ms; ++cnt; }
    }
    ARGCHK(cnt > 0, "no fc1 launch was timed");
    *avg_us = (float)(tot * 1000.0 / cnt);
    *launches = cnt;
    return PPDE_OK;
}

// Diagnostics: an activation of the LAST stateless transformer evaluation (ppde_energy_grad with bit 2) as fp32.
int ppde_debug_transformer_read(ppde_model* m, int what, int layer, float* out_host, int64_t count) {
    ARGCHK(m && m->tf && m->s_tfw && out_host && count >= 0, "no transformer evaluation to read from");
    ARGCHK(layer >= 0 && layer < m->tf->layers, "layer out of range");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipDeviceSynchronize());
    const TfWork* w = m->s_tfw;
    const TfLayerAct& a = w->act[layer];
    const half_t* src = nullptr;
    switch (what) {
        case 0: src = a.xin; break;
        case 1: src = a.qkv; break;
        case 2: return fail(PPDE_ERR_INVALID, "the attention probabilities are not kept (the backward rebuilds them)");
        case 3: src = a.xmid; break;
        case 4: src = a.hpre; break;
        case 5: src = w->xlast; break;
        case 6: src = w->logits; break;
        case 7: src = w->dlogits; break;
        case 8: src = w->gA; break;
        case 9: src = w->G33; break;
        case 10: src = w->ctx; break;
        case 11: src = w->dqkv; break;
        default: return fail(PPDE_ERR_INVALID, "unknown buffer id");
    }
    // the workspace holds ONE chunk of chains (after a chunked evaluation: the last chunk); nothing beyond its buffers is read
    const int D = m->tf->D, F = m->tf->F;
    const size_t width = what == 1 || what == 11 ? (size_t)3 * D : what == 4 ? (size_t)F : (what == 6 || what == 7 || what == 9) ? (size_t)TF_VOCAB_PAD : (size_t)D;
    ARGCHK((uint64_t)count <= (uint64_t)w->M_pad * width, "count exceeds the buffer (the workspace holds one chunk of chains: rows of the last chunk evaluated)");
    std::vector<half_t> h((size_t)count);
    HIPCHK(hipMemcpy(h.data(), src, (size_t)count * sizeof(half_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; ++i) out_host[i] = (float)h[(size_t)i];
    return PPDE_OK;
}

int ppde_model_get_transformer_wt_score(ppde_model* m, float* out_host) {
    ARGCHK(m && out_host, "null argument");
    ARGCHK(m->tf, "no transformer expert");
    *out_host = m->tf->wt_score;
    return PPDE_OK;
}

static int set_potts_body(ppde_model* m, const float* J, const float* h, int Lp, int win_start) {
    set_geom(m, Lp, win_start);
    free_scratch(m);
    int rc = upload_wt(m);
    if (rc) return rc;
    const Geom& g = m->g;
    const size_t nJ = (size_t)Lp * Lp * 400;
    DevBuf<float> raw;
    HIPCHK(raw.alloc(nJ));
    HIPCHK(hipMemcpy(raw.p, J, nJ * sizeof(float), hipMemcpyHostToDevice));
    const size_t nJt = (size_t)Lp * 5 * g.NC * 320;           // float4s
    HIPCHK(dalloc(&m->d_Jt, nJt));
    HIPCHK(dalloc(&m->d_h, (size_t)Lp * 20));
    HIPCHK(hipMemcpy(m->d_h, h, (size_t)Lp * 20 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(potts_prepare_kernel, dim3(1024), dim3(256), 0, 0, raw.p, (float*)m->d_Jt, Lp, g.NC);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    // wt_H = H(wild type) with the same kernel that evaluates every other state
    DevBuf<float> grad, ep, e;
    HIPCHK(grad.alloc((size_t)g.N));
    HIPCHK(ep.alloc((size_t)Lp));
    HIPCHK(e.alloc(1));
    EvalTargets t{grad.p, ep.p, nullptr, nullptr, 0};
    rc = launch_potts(m, States{m->d_wt, m->d_wtT, potts_t4_pad(1)}, 1, t, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(potts_energy_finalize_kernel, dim3(1), dim3(64), 0, 0, ep.p, Lp, 0.0f, e.p, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&m->wt_H, e.p, sizeof(float), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_model_set_potts(ppde_model* m, const float* J, const float* h, int Lp, int win_start) {
    ARGCHK(m && J && h, "null argument");
    ARGCHK(Lp >= 1 && win_start >= 0 && win_start + Lp <= m->L, "Potts window does not fit the sequence");
    // (the ring kernel walks at most 32 chunks of 16 residues; refused before the model is touched)
    ARGCHK(Lp <= 512, "Potts window longer than 512 residues (Lp <= 512)");
    HIPCHK(hipSetDevice(m->device));
    m->has_potts = false;
    if (m->d_Jt) { hipFree(m->d_Jt); m->d_Jt = nullptr; }
    if (m->d_h) { hipFree(m->d_h); m->d_h = nullptr; }
    const int rc = set_potts_body(m, J, h, Lp, win_start);
    if (rc) {
        // no half-set expert: no window, the wild type in the layout of a model without one (the first failure is what is reported)
        const std::string why = g_err;
        if (m->d_Jt) { hipFree(m->d_Jt); m->d_Jt = nullptr; }
        if (m->d_h) { hipFree(m->d_h); m->d_h = nullptr; }
        m->wt_H = 0.f;
        set_geom(m, 0, 0);
        free_scratch(m);
        upload_wt(m);
        return fail(rc, why);
    }
    m->has_potts = true;
    return PPDE_OK;
}

int ppde_model_get_wt_hamiltonian(ppde_model* m, float* out_host) {
    ARGCHK(m && out_host, "null argument");
    ARGCHK(m->has_potts, "no Potts expert");
    *out_host = m->wt_H;
    return PPDE_OK;
}

int ppde_model_set_cnn(ppde_model* m, int n_nets, int C, int K, int F, const float* const* conv_w,
                       const float* const* conv_b, const float* const* lin_w, const float* const* lin_b,
                       const float* const* dec_w, const float* const* dec_b) {
    ARGCHK(m && conv_w && conv_b && lin_w && lin_b && dec_w && dec_b, "null argument");
    ARGCHK(n_nets >= 1 && n_nets <= 4, "1..4 networks supported");
    ARGCHK(K >= 1 && K <= CNN_MAX_K && K <= m->L && C >= 1 && F >= 1, "bad CNN shape (kernel size 1..8)");
    {
        // a shape neither launch form serves is refused here, where it is known, before the model is touched
        const int kt = (K == 5) ? 5 : CNN_MAX_K, cp = (C + 4 * CNN_KB - 1) / (4 * CNN_KB) * (4 * CNN_KB), fp = (F + 15) & ~15;
        if (!cnn_single_launch_shape(m->L - K + 1, cp, fp, kt * 20, m->L)) {
            const std::string why = cnn_chunk_refusal(C, cp, F, fp, kt * 20);
            ARGCHK(why.empty(), why);
        }
    }
    HIPCHK(hipSetDevice(m->device));
    for (void* p : m->cnn_allocs) hipFree(p);
    m->cnn_allocs.clear();
    m->has_cnn = false;
    m->n_nets = n_nets; m->C = C; m->K = K; m->F = F; m->T = m->L - K + 1;
    m->KT = (K == 5) ? 5 : CNN_MAX_K;            // tables hold KT taps (zero padded beyond K)
    m->J = m->KT * 20;
    const int KT = m->KT;
    const int CP = (C + 4 * CNN_KB - 1) / (4 * CNN_KB) * (4 * CNN_KB);   // contraction length: whole B bursts
    m->CP = CP;
    const int FP = (F + 15) & ~15, JP = (m->J + 15) & ~15;
    m->FP = FP; m->JP = JP;
    // what the split-precision kernels take for granted: whole k steps of 32 channels, whole strips of 16 columns
    ARGCHK(CP % 32 == 0 && FP % 16 == 0 && JP % 16 == 0, "padded CNN shape is not a whole number of MFMA blocks");
    auto up = [&](const std::vector<float>& v, const float** out) -> int {
        float* d = nullptr;
        HIPCHK(dalloc(&d, v.size()));
        HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        m->cnn_allocs.push_back(d);
        *out = d;
        return PPDE_OK;
    };
    for (int k = 0; k < n_nets; ++k) {
        CnnNet& nt = m->nets[k];
        std::vector<float> WcT((size_t)KT * 20 * CP, 0.f), bc(CP, 0.f), WeT((size_t)CP * FP, 0.f), We((size_t)FP * CP, 0.f),
            Wf((size_t)CP * JP, 0.f), be(FP, 0.f), wd(FP, 0.f);
        for (int o = 0; o < C; ++o) {
            bc[o] = conv_b[k][o];
            for (int c = 0; c < 20; ++c)
                for (int kp = 0; kp < K; ++kp) {
                    const float w = conv_w[k][((size_t)o * 20 + c) * K + kp];
                    WcT[((size_t)kp * 20 + c) * CP + o] = w;
                    Wf[(size_t)o * JP + (kp * 20 + c)] = w;
                }
        }
        for (int f = 0; f < F; ++f) {
            be[f] = lin_b[k][f];
            wd[f] = dec_w[k][f];
            for (int o = 0; o < C; ++o) {
                const float w = lin_w[k][(size_t)f * C + o];
                We[(size_t)f * CP + o] = w;
                WeT[(size_t)o * FP + f] = w;
            }
        }
        const float* p;
        int rc;
        if ((rc = up(WcT, &p))) return rc; nt.WcT = p;
        if ((rc = up(bc, &p))) return rc; nt.bc = p;
        if ((rc = up(WeT, &p))) return rc; nt.WeT = p;
        if ((rc = up(We, &p))) return rc; nt.We = p;
        if ((rc = up(be, &p))) return rc; nt.be = p;
        if ((rc = up(wd, &p))) return rc; nt.wd = p;
        if ((rc = up(Wf, &p))) return rc; nt.Wf = p;
        // static bounds per channel o -> the power-of-two scales of the two-term fp16 split (cnn.h; all 1 with the bf16 split):
        //   |pre1[t][o]| <= |bc[o]| + sum_tap max_letter |Wc[o][letter][tap]|                            -> sch[o]
        //   |routed gradient[t][o]| <= |scale| sum_f |wd[f] We[f][o]|  (every feature in one row)         -> scg[o] (times CnnArgs.gsc)
        // and, with the inverse channel scales folded in, one scale per weight matrix from its largest entry
        std::vector<float> sch(CP, 1.f), scg(CP, 1.f), WeG((size_t)FP * CP, 0.f);
        double we_max = 0.0, wf_max = 0.0;
        for (int o = 0; o < C; ++o) {
            float hb = fabsf(conv_b[k][o]), wc = 0.f, gb = 0.f, we = 0.f;
            for (int kp = 0; kp < K; ++kp) {
                float mx = 0.f;
                for (int c = 0; c < 20; ++c) mx = fmaxf(mx, fabsf(conv_w[k][((size_t)o * 20 + c) * K + kp]));
                hb += mx;
                wc = fmaxf(wc, mx);
            }
            for (int f = 0; f < F; ++f) {
                const float w = lin_w[k][(size_t)f * C + o];
                gb += fabsf(dec_w[k][f] * w);
                we = fmaxf(we, fabsf(w));
            }
            sch[o] = bf_scale_for(hb);
            scg[o] = bf_scale_for(gb);
            we_max = fmax(we_max, (double)we / sch[o]);
            wf_max = fmax(wf_max, (double)wc / scg[o]);
            for (int f = 0; f < F; ++f) WeG[(size_t)f * CP + o] = We[(size_t)f * CP + o] * scg[o];
        }
        const float sc_we = bf_scale_for((float)we_max), sc_wf = bf_scale_for((float)wf_max);
        nt.un_f = 1.f / sc_we;
        nt.un_b = 1.f / sc_wf;
        if ((rc = up(sch, &p))) return rc; nt.sch = p;
        if (BFT == 2) { if ((rc = up(WeG, &p))) return rc; nt.WeG = p; }
        else nt.WeG = nt.We;
        // the contraction operands with the inverse channel scales and the matrix's own scale applied (exact: powers of two)
        std::vector<float> WeTs(WeT), Wfs(Wf);
        for (int o = 0; o < C; ++o) {
            for (int f = 0; f < FP; ++f) WeTs[(size_t)o * FP + f] = (float)((double)WeT[(size_t)o * FP + f] / sch[o] * sc_we);
            for (int j = 0; j < JP; ++j) Wfs[(size_t)o * JP + j] = (float)((double)Wf[(size_t)o * JP + j] / scg[o] * sc_wf);
        }
        // those two matrices as MFMA B fragments of their split (cnn.h bf_strips):
        // [strip of 16 columns][k step of 32][term][lane] x 8 values of 16 bits, lane = (column l & 15, k = 8 (l >> 4) + j)
        auto frags = [&](const std::vector<float>& W, int ldw, int ncols, const uint4** out) -> int {   // W[k][col], k < CP
            const int KS = CP / 32, NS = ncols / 16;
            std::vector<uint16_t> fr((size_t)NS * KS * BFT * 64 * 8, 0);
            for (int ct = 0; ct < NS; ++ct)
                for (int ks = 0; ks < KS; ++ks)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            uint16_t tt[BFT];
                            bf_split_host(W[(size_t)(ks * 32 + 8 * (l >> 4) + j) * ldw + ct * 16 + (l & 15)], tt);
                            for (int t = 0; t < BFT; ++t) fr[((((size_t)ct * KS + ks) * BFT + t) * 64 + l) * 8 + j] = tt[t];
                        }
            uint16_t* d = nullptr;
            HIPCHK(dalloc(&d, fr.size()));
            HIPCHK(hipMemcpy(d, fr.data(), fr.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            m->cnn_allocs.push_back(d);
            *out = (const uint4*)d;
            return PPDE_OK;
        };
        if ((rc = frags(WeTs, FP, FP, &nt.WeB))) return rc;
        if ((rc = frags(Wfs, JP, JP, &nt.WfB))) return rc;
        {
            // the convolution table as MFMA A fragments of its split, row o scaled by sch[o]: the matrix-pipe convolution produces sch[o] * pre1
            // (cnn.h conv_tile_rows: the convolution of a one-hot input as [channels x (tap, letter)] x [(tap, letter) x rows], one k
            // step of 32 per tap, letters 20..31 zero):
            // [channel tile of 16][tap][term][lane] x 8 values, lane = (channel ct * 16 + (l & 15), letters 8 (l >> 4) + j)
            const int NT16 = CP / 16;
            std::vector<uint16_t> fr((size_t)NT16 * KT * BFT * 64 * 8, 0);
            for (int ct = 0; ct < NT16; ++ct)
                for (int kp = 0; kp < K; ++kp)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int o = ct * 16 + (l & 15), c = 8 * (l >> 4) + j;
                            if (o >= C || c >= 20) continue;
                            uint16_t tt[BFT];
                            bf_split_host(sch[o] * conv_w[k][((size_t)o * 20 + c) * K + kp], tt);
                            for (int t = 0; t < BFT; ++t) fr[((((size_t)ct * KT + kp) * BFT + t) * 64 + l) * 8 + j] = tt[t];
                        }
            uint16_t* d = nullptr;
            HIPCHK(dalloc(&d, fr.size()));
            HIPCHK(hipMemcpy(d, fr.data(), fr.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            m->cnn_allocs.push_back(d);
            nt.WcA = (const uint4*)d;
        }
        nt.bd = dec_b[k][0];
    }
    free_scratch(m);
    hipFree(m->cnn_cmax); hipFree(m->cnn_carg); hipFree(m->cnn_cgate);
    m->cnn_cmax = nullptr; m->cnn_carg = nullptr; m->cnn_cgate = nullptr; m->cnn_scratch_n = 0;
    m->has_cnn = true;
    return PPDE_OK;
}

// ---------------------------------------------------------------------------------------------
static int ensure_scratch(ppde_model* m, int n) {
    if (!m->s_flag) {
        HIPCHK(dalloc(&m->s_flag, 1));
        HIPCHK(hipMemset(m->s_flag, 0, sizeof(int)));
    }
    if (n <= m->scratch_n) return PPDE_OK;
    free_scratch(m);
    const Geom& g = m->g;
    HIPCHK(dalloc(&m->s_state, (size_t)n * g.Ls));
    if (g.Lp > 0) {
        const size_t words = potts_t4_words(g.NC, potts_t4_pad(n));
        HIPCHK(dalloc(&m->s_stateT, words));
        HIPCHK(hipMemset(m->s_stateT, 0, words * sizeof(uint32_t)));
    }
    HIPCHK(dalloc(&m->s_grad, (size_t)n * g.N));
    HIPCHK(hipMemset(m->s_grad, 0, (size_t)n * g.N * sizeof(float)));
    HIPCHK(dalloc(&m->s_epart, (size_t)n * std::max(g.Lp, 1)));
    if (m->has_cnn) {
        HIPCHK(dalloc(&m->s_gradC, (size_t)cnn_parts(m) * n * g.N));
        HIPCHK(dalloc(&m->s_fitC, (size_t)cnn_parts(m) * n));
    }
    m->scratch_n = n;
    return PPDE_OK;
}

int ppde_onehot_to_idx(ppde_model* m, const float* x_dev, int n, uint8_t* idx_dev, void* stream) {
    ARGCHK(m && x_dev && idx_dev && n >= 0, "bad argument");
    if (n == 0) return PPDE_OK;
    HIPCHK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_scratch(m, 1);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(m->s_flag, 0, sizeof(int), s));
    const int tot = n * m->L;
    hipLaunchKernelGGL(k_onehot_to_idx, dim3((tot + 255) / 256), dim3(256), 0, s, x_dev, idx_dev, n, m->L, m->L, 0, m->s_flag);
    HIPCHK(hipGetLastError());
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, m->s_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return fail(PPDE_ERR_NOT_ONEHOT, "input is not one-hot: every residue row must hold exactly one 1.0 and nineteen 0.0");
    return PPDE_OK;
}

int ppde_idx_to_onehot(ppde_model* m, const uint8_t* idx_dev, int n, float* x_dev, void* stream) {
    ARGCHK(m && x_dev && idx_dev && n >= 0, "bad argument");
    if (n == 0) return PPDE_OK;
    HIPCHK(hipSetDevice(m->device));
    const int tot = n * m->L * 20;
    hipLaunchKernelGGL(k_idx_to_onehot, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx_dev, x_dev, n, m->L, m->L, 0);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

int ppde_energy_grad(ppde_model* m, const uint8_t* idx_dev, int n, int which, float* e_dev, float* fit_dev,
                     float* grad_dev, void* stream) {
    ARGCHK(m && idx_dev && n >= 0, "bad argument");
    ARGCHK(which >= 1 && which <= 15 && (which & 7), "which: bit 0 Potts, bit 1 supervised, bit 2 transformer expert, bit 3 full gradient");
    // (an energy whose expert was never set is refused before scratch is allocated or a kernel goes out)
    ARGCHK(!(which & 1) || m->has_potts, "the energy uses the Potts expert but ppde_model_set_potts was not called");
    ARGCHK(!(which & 2) || m->has_cnn, "the energy uses the supervised expert but ppde_model_set_cnn was not called");
    ARGCHK(!(which & 4) || m->tf, "no transformer expert");
    if (n == 0) return PPDE_OK;
    HIPCHK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_scratch(m, n);
    if (rc) return rc;
    if ((which & 2) && m->has_cnn && (rc = ensure_cnn_scratch(m, n))) return rc;
    const Geom& g = m->g;
    hipLaunchKernelGGL(k_pack_state, dim3((n * g.Ls + 255) / 256), dim3(256), 0, s, idx_dev, m->s_state, n, g.L, g.Ls, g.sh);
    HIPCHK(hipGetLastError());
    const States st{m->s_state, m->s_stateT, potts_t4_pad(m->scratch_n)};
    if ((which & 1) && (rc = state_rows_to_t4(m, m->s_state, m->s_stateT, n, st.n_pad, s))) return rc;
    EvalTargets t{m->s_grad, m->s_epart, m->s_gradC, m->s_fitC, 0};
    if (which & 4) {
        ARGCHK(m->tf, "no transformer expert");
        if (!m->s_tfw || m->s_tfw->n_cap < std::min(n, tf_chunk_cap(m->tf))) {      // activations: one chunk of chains
            delete m->s_tfw; m->s_tfw = nullptr;
            m->s_tfw = new TfWork();
            if ((rc = tf_alloc_work(m->tf, m->s_tfw, n)) != PPDE_OK) {                 // leave no half-built workspace behind
                delete m->s_tfw; m->s_tfw = nullptr;
                return rc;
            }
        }
        if (m->s_tf_n < n) {                                                         // gradient rows and scores: all n chains
            hipFree(m->s_gradT); hipFree(m->s_tfE); m->s_gradT = m->s_tfE = nullptr; m->s_tf_n = 0;
            if (dalloc(&m->s_gradT, (size_t)n * g.N) != hipSuccess || dalloc(&m->s_tfE, (size_t)n) != hipSuccess) {
                hipFree(m->s_gradT); hipFree(m->s_tfE); m->s_gradT = m->s_tfE = nullptr;
                return fail(PPDE_ERR_HIP, "device allocation failed for the transformer gradient rows");
            }
            m->s_tf_n = n;
        }
        t.gradT = m->s_gradT; t.tfE = m->s_tfE; t.tfw = m->s_tfw;
    }
    t.cmax = m->cnn_cmax; t.carg = m->cnn_carg; t.cgate = m->cnn_cgate; t.cnn_cap = m->cnn_scratch_n;
    // the scratch is laid out for scratch_n chains; kernels index slot 0 with stride n, which is fine for slot 0
    rc = eval_experts(m, which, st, n, t, grad_dev != nullptr, s);
    if (rc) return rc;
    PasArgs a = base_pas_args(m, which, n);
    a.grad = m->s_grad; a.epart = m->s_epart; a.gradC = m->s_gradC; a.fitC = m->s_fitC;
    a.gradT = m->s_gradT; a.tfE = m->s_tfE;
    if (e_dev || fit_dev) {
        hipLaunchKernelGGL(k_slot_energy, dim3((n + 3) / 4), dim3(256), 0, s, a, e_dev, fit_dev);
        HIPCHK(hipGetLastError());
    }
    if (grad_dev) {
        hipLaunchKernelGGL(k_combine_rows, dim3(n), dim3(256), 0, s, a, grad_dev);
        HIPCHK(hipGetLastError());
    }
    return PPDE_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------
#include "chains.h"

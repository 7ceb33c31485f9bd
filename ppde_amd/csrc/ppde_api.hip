// Host side of the C ABI declared in include/ppde_hip.h: device memory ownership, weight re-layout,
// kernel launches, hipGraph capture of the iteration loop.
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
    HIPCHK(hipSetDevice(m->device));
    delete m->tf; m->tf = nullptr;
    delete m->s_tfw; m->s_tfw = nullptr;
    hipFree(m->s_gradT); hipFree(m->s_tfE); m->s_gradT = m->s_tfE = nullptr; m->s_tf_n = 0;
    TfModel* t = new TfModel();
    t->layers = n_layers; t->Dr = dim; t->D = (dim + 127) & ~127; t->H = heads; t->F = ffn; t->HD = dim / heads;
    int rc = tf_build_model(t, m->L, w);
    if (rc) { delete t; return rc; }
    // wild type's local score (nets.py:188) with the kernels that evaluate every other state
    TfWork wk;
    DevBuf<float> sc;
    if ((rc = tf_alloc_work(t, &wk, 1)) == PPDE_OK && sc.alloc(1) != hipSuccess) rc = fail(PPDE_ERR_HIP, "allocation failed");
    if (rc == PPDE_OK) rc = tf_eval(t, &wk, m->d_wt, m->g.Ls, m->g.sh, 1, sc.p, nullptr, 0);
    if (rc == PPDE_OK && hipMemcpy(&t->wt_score, sc.p, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(PPDE_ERR_HIP, "copy failed");
    if (rc) { delete t; return rc; }
    m->tf = t;
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
// The optional modes of a chains object, one struct each: what the mode was set with, its device buffers and the sizes that follow
// from them. A mode is on while it holds its buffers. ppde_chains_set_* builds a local one and moves it into the object once
// everything is allocated (a failure on the way leaves the object as it was and the local's destructor releases what there is);
// assigning {} clears it.

// parallel tempering (ppde_chains_set_tempering)
struct Tempering {
    int n_rungs = 0, swap_every = 0;
    std::vector<float> ladder;                   // beta[0] > beta[1] > ... > 0
    DevBuf<float> beta;                          // [n]
    DevBuf<int> rung, slot;                      // [n], [n/R][R]
    DevBuf<long long> swap_attempts, swap_accepts;   // [n/R][R-1]
    DevBuf<uint8_t> rung_hist;                   // [T+1][n]
    bool on() const { return beta.p != nullptr; }
};

// population annealing (ppde_chains_set_annealing, ppde_chains_set_annealing_adaptive)
struct Annealing {
    int D = 0, every = 0, S = 0, cap = 0;        // deme size, iterations per stage, stages (adaptive: max_stages), events_cap
    std::vector<float> sched;                    // beta[0] <= ... <= beta[S] (adaptive: beta_start, beta_end)
    DevBuf<float> sched_dev, beta, pre;          // [S+1] (adaptive: [2]), [n], [events_cap][n]
    bool adaptive = false;                       // the deme chooses each step (k_select_plan_adaptive)
    float rho = 0.f, min_step = 0.f;             // its ESS target and its smallest step
    DevBuf<float> beta_pair;                     // [2][events_cap][n/D] beta before / after every event (adaptive only)
    DevBuf<int> parent;                          // [events_cap][n]
    DevBuf<double> lmw, ess;                     // [events_cap][n/D]
    bool on() const { return sched_dev.p != nullptr; }
    int events_done(int steps_done) const { return std::min(cap, steps_done / every); }
};

// recombination (ppde_chains_set_recombination)
struct Recombination {
    int D = 0, every = 0, cap = 0;               // deme size, iterations per event, events_cap
    std::vector<int32_t> open;                   // the open list: residues of [min_pos, max_pos] the library leaves open, increasing
    DevBuf<int> open_dev;                        // [n_open]
    DevBuf<int> partner, lo, hi, differ, child_dist;   // [events_cap][n] each
    DevBuf<uint8_t> outcome;
    DevBuf<float> log_ratio, pre, child;
    bool on() const { return open_dev.p != nullptr; }
    int events_done(int steps_done) const { return std::min(cap, steps_done / every); }
    bool event(int it) const { return (it + 1) % every == 0; }   // (it: absolute, or relative to a multiple of every)
};

// recorder (ppde_chains_set_recorder)
struct Recorder {
    ppde_record_config cfg{};
    int rows_cap = 0, slots = 0;
    DevBuf<uint8_t> idx;                         // [rows_cap][slots][Ls] (keep_samples)
    DevBuf<float> e, f;                          // [rows_cap][slots]
    DevBuf<int> chain;
    DevBuf<unsigned long long> counts;           // [L][20]
    bool on() const { return counts.p != nullptr; }
    int rows_done(int steps_done) const { return steps_done > cfg.burn_in ? (steps_done - cfg.burn_in) / cfg.every : 0; }
};

// pair counts (ppde_chains_set_pair_counts)
struct PairCounts {
    std::vector<int32_t> sites;                  // [S] residues, strictly increasing
    int nt = 0;                                  // tiles per side (pairs.h)
    DevBuf<int> sites_dev;                       // [nt * PAIR_TS], padded with -1
    DevBuf<unsigned long long> counts;           // [nt (nt + 1) / 2][PAIR_TILE]
    bool on() const { return counts.p != nullptr; }
    size_t tiles() const { return (size_t)nt * ((size_t)nt + 1) / 2; }
};

// archive (ppde_chains_set_archive)
struct Archive {
    int k = 0;
    DevBuf<uint8_t> idx;                         // [n][K][Ls]
    DevBuf<float> e, f;                          // [n][K]
    DevBuf<int> step, count;                     // [n][K], [n]
    DevBuf<unsigned int> hash;                   // [n][K] fingerprints (archive.h)
    bool on() const { return idx.p != nullptr; }
};

// move statistics (ppde_chains_set_stats)
struct MoveStats {
    int n = 0, R = 1, M = 0, L = 0, per_site = 0;   // the shape at the set call: chains, R' = max(n_rungs, 1), path lengths, residues
    DevBuf<long long> cnt;                       // six [n][R'], two [R'][M], then [R'][L] with per_site (counter)
    DevBuf<uint8_t> prev;                        // [2][n][Ls] the state the last counted iteration left, read and written in turns (stats.h)
    DevBuf<int> dist;                            // [n]     its mutation count
    bool on() const { return cnt.p != nullptr; }
    // the counters in one allocation: k = 0..5 iters, accepts, moved, jump_sum, dist_sum, wt_returns [n][R'];
    // 6, 7 len_attempts, len_accepts [R'][M]; 8 site_changes [R'][L]
    size_t cells(int k) const { return k < 6 ? (size_t)n * R : k < 8 ? (size_t)R * M : per_site ? (size_t)R * L : 0; }
    size_t cells_before(int k) const {
        size_t o = 0;
        for (int j = 0; j < k; ++j) o += cells(j);
        return o;
    }
    long long* counter(int k) const { return cnt + cells_before(k); }
    size_t cells_total() const { return cells_before(9); }
};

struct ppde_chains {
    ppde_model* m = nullptr;
    int device = 0;                              // (kept here: destroy must not depend on the model still being alive)
    ppde_chain_config cfg{};
    hipStream_t stream = nullptr;                // == streams[0]
    std::vector<hipStream_t> streams;            // one per sub-population
    std::vector<hipEvent_t> events;              // fork (0) / join (1..) markers
    std::vector<int> sub_off, sub_n;             // sub-population k covers chains [sub_off[k], sub_off[k] + sub_n[k])
    int n = 0, T = 0, mu_max = 1, steps_done = 0;
    bool initialised = false;
    // device buffers
    uint32_t *curT = nullptr, *propT = nullptr;  // T4 copies of cur / prop (potts.h), n_pad chains per row
    int n_pad = 0;
    uint8_t *cur = nullptr, *prop = nullptr, *fb_state = nullptr, *best_state = nullptr,
            *rtraj = nullptr, *tmp_acc = nullptr, *tr_acc = nullptr, *tmp_idx = nullptr;
    unsigned char* rec = nullptr;                // [n] chain records
    int rec_stride = 0;
    float wt_e = 0.f, wt_f = 0.f;                // wild type's energy / fitness (mutation-cap reset under gradient reuse)
    float *grad_cur = nullptr, *grad = nullptr, *epart = nullptr, *gradC = nullptr, *fitC = nullptr,
          *fb_grad = nullptr, *fb_e = nullptr, *fb_f = nullptr, *e_hist = nullptr,
          *f_hist = nullptr, *tmp_be = nullptr, *tmp_bf = nullptr, *tr_logacc = nullptr;
    int* h_err = nullptr;                        // pinned, device-mapped host word behind err_flag: the sync reads it without a copy
    long long d_it_val = -1;                     // value the device iteration counter holds (-1: unknown)
    int *tmp_bt = nullptr, *tr_flat = nullptr, *tr_U = nullptr, *err_flag = nullptr,
        *d_it = nullptr, *tmp_dist = nullptr;
    unsigned long long* dbg = nullptr;           // stamps of the diagnostic build (64 x (cycles, 100 MHz ticks))
    // transformer expert: this object's activation workspace, gradient rows [2][n][N] and scores [2][n]
    TfWork* tfw = nullptr;
    float *gradT = nullptr, *tfE = nullptr;
    // chunk scratch of the long-sequence CNN path (this object's own: its graphs hold these pointers)
    float* cnn_cmax = nullptr;
    int* cnn_carg = nullptr;
    uint32_t* cnn_cgate = nullptr;
    // graph replay: segments of different lengths, longest first, captured once by ppde_chains_init
    struct GraphSeg { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; int len = 0; };
    std::vector<GraphSeg> graphs;
    int n_captures = 0, n_captures_in_run = 0;   // graphs captured in all / inside ppde_chains_run (must stay 0)
    long long n_replayed_steps = 0, n_eager_steps = 0;
    std::vector<void*> allocs;
    DevBuf<uint32_t> allowed;                    // design library [L] (ppde_chains_set_library); NULL = none
    bool reversible = false;                     // ppde_chains_set_reversible: the accept phases run the *_rev kernels
    Tempering temper;
    Annealing anneal;
    Recombination recomb;
    Recorder recorder;
    PairCounts pairs;
    Archive archive;
    MoveStats stats;

    ppde_chains() = default;
    ppde_chains(const ppde_chains&) = delete;
    ppde_chains& operator=(const ppde_chains&) = delete;
    // everything the object owns; the members (the modes' buffers) go after the body, with this device current
    ~ppde_chains() {
        hipSetDevice(device);
        for (auto& gs : graphs) {
            if (gs.exec) hipGraphExecDestroy(gs.exec);
            if (gs.graph) hipGraphDestroy(gs.graph);
        }
        for (void* p : allocs) hipFree(p);
        delete tfw;
        if (h_err) hipHostFree(h_err);
        for (hipStream_t st : streams) if (st) hipStreamDestroy(st);
        for (hipEvent_t ev : events) if (ev) hipEventDestroy(ev);
    }
};

static PasArgs chain_args(const ppde_chains* c) {
    const ppde_model* m = c->m;
    PasArgs a = base_pas_args(m, c->cfg.which, c->n);
    a.pas = c->cfg.pas_length;
    a.thr = c->cfg.nmut_threshold == 0 ? 0x7fffffff : c->cfg.nmut_threshold;
    a.paper = c->cfg.paper_results; a.min_pos = c->cfg.min_pos; a.max_pos = c->cfg.max_pos;
    a.rng_mode = c->cfg.rng_mode; a.reuse = c->cfg.reuse_grad; a.rec_after_reset = c->cfg.record_after_reset;
    a.random_chain = c->cfg.random_chain; a.mu_max = c->mu_max; a.mu_cap = c->mu_max;
    a.key.k0 = (uint32_t)c->cfg.seed;
    a.key.k1 = (uint32_t)(c->cfg.seed >> 32) ^ (uint32_t)(c->cfg.chain_offset >> 32);
    a.key.chain_lo = (uint32_t)c->cfg.chain_offset;
    a.cur = c->cur; a.prop = c->prop; a.fb_state = c->fb_state;
    a.curT = (uint8_t*)c->curT; a.propT = (uint8_t*)c->propT; a.n_pad = c->n_pad;
    a.fb_state_stride = c->cfg.paper_results ? m->g.Ls : 0;
    a.grad = c->grad; a.epart = c->epart; a.gradC = c->gradC; a.fitC = c->fitC;
    a.gradT = c->gradT; a.tfE = c->tfE;
    a.grad_cur = c->grad_cur; a.rec = c->rec; a.rec_stride = c->rec_stride; a.wt_e = c->wt_e; a.wt_f = c->wt_f;
    a.fb_grad = c->fb_grad; a.fb_grad_stride = c->cfg.paper_results ? (size_t)m->g.N : 0;
    a.e_hist = c->e_hist; a.f_hist = c->f_hist; a.best_state = c->best_state; a.rtraj = c->rtraj;
    a.tr_flat = c->tr_flat; a.tr_acc = c->tr_acc; a.tr_logacc = c->tr_logacc; a.tr_U = c->tr_U;
    a.err_flag = c->err_flag;
    a.dbg = c->dbg;
    a.allowed = c->allowed;
    a.beta = c->anneal.on() ? c->anneal.beta.p : c->temper.beta.p; a.rung = c->temper.rung; a.slot = c->temper.slot; a.swap_attempts = c->temper.swap_attempts; a.swap_accepts = c->temper.swap_accepts;
    a.rung_hist = c->temper.rung_hist; a.n_rungs = c->temper.n_rungs; a.swap_every = c->temper.swap_every;
    return a;
}

// the recorder's kernel for iteration it_base + it_local (record.h): every chain of the object; reads cur, the history rows, slot
static int launch_record(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Geom& g = c->m->g;
    const Recorder& rec = c->recorder;
    RecArgs r{};
    r.it_base = it_base; r.it_local = it_local;
    r.n = c->n; r.L = g.L; r.Ls = g.Ls; r.sh = g.sh;
    r.burn_in = rec.cfg.burn_in; r.every = rec.cfg.every; r.rung = rec.cfg.rung; r.n_rungs = c->temper.n_rungs; r.slots = rec.slots;
    r.cur = c->cur; r.e_hist = c->e_hist; r.f_hist = c->f_hist; r.slot = c->temper.slot;
    r.idx = rec.idx; r.energy = rec.e; r.fitness = rec.f; r.chain = rec.chain; r.counts = rec.counts;
    hipLaunchKernelGGL(k_record, dim3(((g.Ls >> 2) + 3) / 4), dim3(REC_BLOCK), 0, s, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// the pair counts' kernel for the same iteration (pairs.h), on the recorder's schedule and slots; reads cur and slot only
static int launch_pairs(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Geom& g = c->m->g;
    const Recorder& rec = c->recorder;
    PairArgs p{};
    p.it_base = it_base; p.it_local = it_local; p.Ls = g.Ls; p.sh = g.sh;
    p.burn_in = rec.cfg.burn_in; p.every = rec.cfg.every; p.rung = rec.cfg.rung; p.n_rungs = c->temper.n_rungs; p.slots = rec.slots;
    p.nt = c->pairs.nt; p.cur = c->cur; p.slot = c->temper.slot; p.sites = c->pairs.sites_dev; p.counts = c->pairs.counts;
    hipLaunchKernelGGL(k_record_pairs, dim3((unsigned)c->pairs.tiles()), dim3(PAIR_BLOCK), 0, s, p);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// the archive's kernel for the state after it_base + it_local + 1 completed iterations (archive.h): every chain of the object
static int launch_archive(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Geom& g = c->m->g;
    ArchArgs r{};
    r.it_base = it_base; r.it_local = it_local;
    r.n = c->n; r.K = c->archive.k; r.L = g.L; r.Ls = g.Ls; r.sh = g.sh;
    r.rec = c->rec; r.rec_stride = c->rec_stride; r.cur = c->cur; r.e_hist = c->e_hist; r.f_hist = c->f_hist;
    r.idx = c->archive.idx; r.energy = c->archive.e; r.fitness = c->archive.f; r.step = c->archive.step; r.count = c->archive.count;
    r.hash = c->archive.hash;
    hipLaunchKernelGGL(k_archive, dim3((c->n + ARCH_BLOCK / 64 - 1) / (ARCH_BLOCK / 64)), dim3(ARCH_BLOCK), 0, s, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// the statistics' kernel for iteration it_base + it_local (stats.h): every chain of the object. U / mu_cap: the caller-supplied
// path lengths of that iteration and the sub-steps its noise covers (rng_mode 0)
static int launch_stats(ppde_chains* c, const int* it_base, int it_local, const int* U, int mu_cap, hipStream_t s) {
    const Geom& g = c->m->g;
    StatArgs r{};
    r.it_base = it_base; r.it_local = it_local;
    r.n = c->n; r.R = c->stats.R; r.M = c->mu_max; r.L = g.L; r.Ls = g.Ls; r.sh = g.sh;
    r.rng_mode = c->cfg.rng_mode; r.pas = c->cfg.pas_length; r.mu_cap = mu_cap > 0 ? mu_cap : c->mu_max;
    r.key = chain_args(c).key;
    r.rec = c->rec; r.rec_stride = c->rec_stride; r.cur = c->cur; r.rung_hist = c->temper.on() ? c->temper.rung_hist.p : nullptr; r.U_in = U;
    r.prev = c->stats.prev; r.pdist = c->stats.dist;
    const MoveStats& st = c->stats;
    r.iters = st.counter(0); r.accepts = st.counter(1); r.moved = st.counter(2); r.jump_sum = st.counter(3);
    r.dist_sum = st.counter(4); r.wt_returns = st.counter(5);
    r.len_attempts = st.counter(6); r.len_accepts = st.counter(7);
    r.site_changes = st.per_site ? st.counter(8) : nullptr;
    r.site_blocks = c->stats.per_site ? ((g.Ls >> 2) + 3) / 4 : 0;
    const size_t lds = std::max(2 * (size_t)r.M, (size_t)16) * r.R * sizeof(unsigned int);   // (at most 64 x 127 x 2 cells: 65 024 bytes)
    hipLaunchKernelGGL(k_stats, dim3(r.site_blocks + (c->n + STAT_NW - 1) / STAT_NW + 1), dim3(STAT_BLOCK), lds, s, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// the two selection kernels behind the accept phase of iteration it_base + it_local (anneal.h): every chain of the object
static int launch_select(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const PasArgs p = chain_args(c);
    AnnealArgs r{};
    r.it_base = it_base; r.it_local = it_local;
    r.n = c->n; r.D = c->anneal.D; r.every = c->anneal.every; r.S = c->anneal.S;
    r.g = p.g; r.n_pad = c->n_pad; r.key = p.key;
    r.rec_stride = c->rec_stride; r.random_chain = c->cfg.random_chain; r.reuse = c->cfg.reuse_grad;
    r.sched = c->anneal.sched_dev; r.beta = c->anneal.beta; r.rec = c->rec; r.cur = c->cur; r.curT = (uint8_t*)c->curT;
    r.grad_cur = c->grad_cur; r.e_hist = c->e_hist; r.f_hist = c->f_hist; r.best_state = c->best_state; r.rtraj = c->rtraj;
    r.parent = c->anneal.parent; r.pre_energy = c->anneal.pre; r.log_mean_w = c->anneal.lmw; r.ess = c->anneal.ess;
    if (c->anneal.adaptive) {
        const AnnealStepArgs x{c->anneal.sched[1], c->anneal.rho, c->anneal.min_step, c->anneal.cap, c->anneal.beta_pair};
        hipLaunchKernelGGL(k_select_plan_adaptive, dim3(c->n / c->anneal.D), dim3(ANNEAL_BLOCK), 0, s, r, x);
    } else {
        hipLaunchKernelGGL(k_select_plan, dim3(c->n / c->anneal.D), dim3(ANNEAL_BLOCK), 0, s, r);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_select_copy, dim3(c->n), dim3(ANNEAL_BLOCK), 0, s, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

static States cur_states(const ppde_chains* c) { return States{c->cur, c->curT, c->n_pad}; }
static States prop_states(const ppde_chains* c) { return States{c->prop, c->propT, c->n_pad}; }
static EvalTargets chain_targets(const ppde_chains* c, int slot) {
    EvalTargets t{c->grad, c->epart, c->gradC, c->fitC, slot, c->dbg};
    t.cmax = c->cnn_cmax; t.carg = c->cnn_carg; t.cgate = c->cnn_cgate; t.cnn_cap = c->n;
    t.gradT = c->gradT; t.tfE = c->tfE; t.tfw = c->tfw;
    return t;
}

// the recombination event behind the accept phase of iteration it_base + it_local (recombine.h): the children of every pair into
// the proposal slot, the run's expert evaluation of that slot, the decision and the hand-over. Every chain of the object.
static int launch_cross(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Recombination& rc = c->recomb;
    CrossArgs r{};
    r.p = chain_args(c);
    r.p.it_base = it_base; r.p.it_local = it_local;
    r.D = rc.D; r.every = rc.every; r.cap = rc.cap; r.n_open = (int)rc.open.size();
    r.open = rc.open_dev; r.partner = rc.partner; r.lo = rc.lo; r.hi = rc.hi; r.differ = rc.differ; r.child_dist = rc.child_dist;
    r.outcome = rc.outcome; r.log_ratio = rc.log_ratio; r.pre_energy = rc.pre; r.child_energy = rc.child;
    hipLaunchKernelGGL(k_cross_propose, dim3(c->n / 2), dim3(CROSS_BLOCK), 0, s, r);
    HIPCHK(hipGetLastError());
    int e = eval_experts(c->m, c->cfg.which, prop_states(c), c->n, chain_targets(c, 1), 1, s, 0, c->n);
    if (e) return e;
    hipLaunchKernelGGL(k_cross_accept, dim3(c->n / 2), dim3(CROSS_BLOCK), 0, s, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

enum ChainKernel { KP_PROPOSE, KP_ACCEPT, KP_ACCEPT_PROPOSE };

static int launch_chain_kernel(ppde_chains* c, ChainKernel which, const PasArgs& a, int n_sub, hipStream_t s) {
    const ppde_model* m = c->m;
    // a run with a design library: the forward paths go to the general *_lib kernels with room for the words in LDS; the
    // accept kernel (no masks on the way back in the default mode) and every run without a library keep their instantiations
    // and LDS size
    // (reversible mode: the reverse rows take the library too, so its accept kernel stages the words as well)
    const bool rev = c->reversible && which != KP_PROPOSE;
    const bool lib = a.allowed != nullptr && (which != KP_ACCEPT || rev);
    const size_t lds = pas_lds_bytes(m->g) + (lib ? pas_lib_lds_bytes(m->g) : 0);
    const int gpt = (m->g.N / 4 + PPDE_BLOCK - 1) / PPDE_BLOCK;
    // specialised instantiation for the common configurations (pas.h pin_config), the general kernel otherwise
    static const bool spec_on = env_int("PPDE_CHAIN_SPEC", 1) != 0;   // tuning knob
    int spec = 0;
    if (spec_on && a.rng_mode == 1 && !a.paper && !a.rec_after_reset && !a.tr_flat && a.which == a.gwhich &&
        (a.which == 1 || a.which == 3))
        spec = (a.which == 1 ? PAS_SPEC_POTTS : PAS_SPEC_POE) | (a.thr == 0x7fffffff ? PAS_SPEC_NOCAP : 0) |
               (which == KP_ACCEPT_PROPOSE ? 0 : a.reuse ? PAS_SPEC_REUSE : PAS_SPEC_REEVAL);
    // (every specialisation the host can ask for is instantiated below: experts x cap x policy; the fused kernel has no policy bit)
    auto with_gpt = [&](auto&& f) {
        switch (gpt) {
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            default: f(std::integral_constant<int, 3>{}); break;
        }
    };
    auto with_spec = [&](auto&& f) {
        switch (spec) {
#define PPDE_SP(v) case (v): f(std::integral_constant<int, (v)>{}); break;
#define PPDE_SP3(b) PPDE_SP(b) PPDE_SP((b) | PAS_SPEC_REEVAL) PPDE_SP((b) | PAS_SPEC_REUSE)
            PPDE_SP3(PAS_SPEC_POTTS) PPDE_SP3(PAS_SPEC_POTTS | PAS_SPEC_NOCAP) PPDE_SP3(PAS_SPEC_POE) PPDE_SP3(PAS_SPEC_POE | PAS_SPEC_NOCAP)
#undef PPDE_SP3
#undef PPDE_SP
            default: f(std::integral_constant<int, 0>{}); break;
        }
    };
    hipEvent_t evs = g_potts_events ? g_potts_events->next(false) : nullptr;       // (in-situ timing: this kernel's end = the next Potts launch's start)
    auto go = [&](auto k) { launch_kernel(k, dim3(n_sub), dim3(PPDE_BLOCK), lds, s, evs, a); };
    with_gpt([&](auto G) {
        constexpr int GP = decltype(G)::value;
        if (c->temper.on() || c->anneal.on()) {          // tempering, annealing (reversible mode): general instantiations, rows and ratio on beta[b] * E
            if (which == KP_PROPOSE) {
                if (a.rng_mode == 0) { if (lib) go(k_propose_temp<GP, true, true>); else go(k_propose_temp<GP, true, false>); }
                else { if (lib) go(k_propose_temp<GP, false, true>); else go(k_propose_temp<GP, false, false>); }
            } else if (a.rng_mode == 1) { if (lib) go(k_accept_temp<GP, true, true>); else go(k_accept_temp<GP, true, false>); }
            else { if (lib) go(k_accept_temp<GP, false, true>); else go(k_accept_temp<GP, false, false>); }
            return;
        }
        if (rev) {                                   // general instantiations only; the forward path keeps its kernels
            if (which == KP_ACCEPT_PROPOSE) { if (lib) go(k_accept_propose_rev<GP, true>); else go(k_accept_propose_rev<GP, false>); }
            else if (a.rng_mode == 1) { if (lib) go(k_accept_rev<GP, true, true>); else go(k_accept_rev<GP, true, false>); }
            else { if (lib) go(k_accept_rev<GP, false, true>); else go(k_accept_rev<GP, false, false>); }
            return;
        }
        if (lib) {
            if (which == KP_ACCEPT_PROPOSE) go(k_accept_propose_lib<GP>);
            else if (a.rng_mode == 0) go(k_propose_lib<GP, true>);
            else go(k_propose_lib<GP, false>);
            return;
        }
        if (which == KP_PROPOSE && a.rng_mode == 0) {
            go(k_propose<GP, true, 0>);
            return;
        }
        with_spec([&](auto S) {
            constexpr int SP = decltype(S)::value;
            constexpr bool policy = (SP & (PAS_SPEC_REEVAL | PAS_SPEC_REUSE)) != 0;
            if (which == KP_ACCEPT_PROPOSE) {
                if constexpr (!policy) go(k_accept_propose<GP, SP>);
            } else if constexpr (policy || SP == 0) {
                if (which == KP_PROPOSE) go(k_propose<GP, false, SP>);
                else if (SP != 0 || a.rng_mode == 1) go(k_accept<GP, SP, true>);
                else go(k_accept<GP, 0, false>);   // replay: the reference's bits
            }
        });
    });
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// `count` iterations of ppde.py:65-153 for sub-population k, enqueued on that sub-population's stream.
// Re-evaluating mode: EG(x) P EG(y) A per iteration. Reuse mode: P, then EG(y) + fused [accept | next propose].
// Tempering: [EG(x)] P EG(y) A S, never fused: the next proposal must see the post-swap beta, the swap the post-accept energy.
// Annealing: the same flow with the two selection kernels in the swap's place.
// Recombination: on the host-chosen event iterations the event's three launches follow a plain accept kernel, and the next iteration
// starts with a plain propose launch (nothing fuses across an event); everywhere else the flow is that of the run without the mode.
static int enqueue_iterations(ppde_chains* c, int k, const int* it_base, int first_local, int count, const int* U,
                              const float* q, const float* u, int mu_cap = 0) {
    const ppde_model* m = c->m;
    hipStream_t s = c->streams[k];
    const int b_off = c->sub_off[k], n_sub = c->sub_n[k];
    PasArgs a = chain_args(c);
    a.b_off = b_off; a.it_base = it_base; a.U_in = U; a.q_in = q; a.u_in = u;
    if (mu_cap > 0) a.mu_cap = mu_cap;              // caller-supplied noise holds only max_u[i] sub-steps of variates
    const bool fuse = c->cfg.reuse_grad && c->cfg.rng_mode == 1 && !c->temper.on() && !c->anneal.on();
    int rc;
    bool after_event = false;                       // the previous iteration of this call ended with a recombination event
    for (int i = 0; i < count; ++i) {
        a.it_local = first_local + i;
        const bool event = c->recomb.on() && c->recomb.event(a.it_local);
        if (!c->cfg.reuse_grad) {   // energy and gradient at the current state (ppde.py:79)
            rc = eval_experts(m, c->cfg.which, cur_states(c), c->n, chain_targets(c, 0), 1, s, b_off, n_sub);
            if (rc) return rc;
        }
        if (!fuse || i == 0 || after_event) {
            rc = launch_chain_kernel(c, KP_PROPOSE, a, n_sub, s);
            if (rc) return rc;
        }
        // energy and gradient at the proposal (ppde.py:119)
        rc = eval_experts(m, c->cfg.which, prop_states(c), c->n, chain_targets(c, 1), 1, s, b_off, n_sub);
        if (rc) return rc;
        rc = launch_chain_kernel(c, (fuse && i + 1 < count && !event) ? KP_ACCEPT_PROPOSE : KP_ACCEPT, a, n_sub, s);
        if (rc) return rc;
        after_event = event;
        // what follows runs on the object's one stream and covers every chain of it: the swap or the selection, then the observers,
        // which see the population those left
        if (c->temper.on()) {
            hipLaunchKernelGGL(k_swap, dim3((c->n + 255) / 256), dim3(256), 0, s, a);
            HIPCHK(hipGetLastError());
        }
        if (c->anneal.on() && (rc = launch_select(c, it_base, a.it_local, s))) return rc;
        if (event && (rc = launch_cross(c, it_base, a.it_local, s))) return rc;
        if (c->recorder.on() && (rc = launch_record(c, it_base, a.it_local, s))) return rc;
        if (c->pairs.on() && (rc = launch_pairs(c, it_base, a.it_local, s))) return rc;      // (set only next to a recorder)
        if (c->archive.on() && (rc = launch_archive(c, it_base, a.it_local, s))) return rc;
        if (c->stats.on() && (rc = launch_stats(c, it_base, a.it_local, U, mu_cap, s))) return rc;
    }
    return PPDE_OK;
}

// `count` iterations starting at (it_base, first_local) for every sub-population: fork from stream 0, run the
// sub-populations' iteration chains side by side, join back on stream 0.
static int enqueue_block(ppde_chains* c, const int* it_base, int first_local, int count) {
    const int K = (int)c->streams.size();
    if (K > 1) {
        HIPCHK(hipEventRecord(c->events[0], c->streams[0]));
        for (int k = 1; k < K; ++k) HIPCHK(hipStreamWaitEvent(c->streams[k], c->events[0], 0));
    }
    for (int k = 0; k < K; ++k) {
        int rc = enqueue_iterations(c, k, it_base, first_local, count, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    for (int k = 1; k < K; ++k) {
        HIPCHK(hipEventRecord(c->events[k], c->streams[k]));
        HIPCHK(hipStreamWaitEvent(c->streams[0], c->events[k], 0));
    }
    return PPDE_OK;
}

// Capture `len` iterations (iteration index = device counter + node-local offset) into a graph segment.
static int capture_segment(ppde_chains* c, int len, bool inside_run) {
    ppde_chains::GraphSeg gs;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_block(c, c->d_it, 0, len);
    if (rc == PPDE_OK) hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, c->stream, c->d_it, len);
    hipError_t e = hipStreamEndCapture(c->stream, &gs.graph);
    if (rc == PPDE_OK && e == hipSuccess) e = hipGraphInstantiate(&gs.exec, gs.graph, nullptr, nullptr, 0);
    if (rc != PPDE_OK || e != hipSuccess) {
        if (gs.exec) hipGraphExecDestroy(gs.exec);
        if (gs.graph) hipGraphDestroy(gs.graph);
        if (rc) return rc;
        return fail(PPDE_ERR_HIP, std::string("hipGraph capture: ") + hipGetErrorString(e));
    }
    hipGraphUpload(gs.exec, c->stream);              // (best effort: the first replay then finds the graph on the device)
    gs.len = len;
    c->graphs.push_back(gs);
    c->n_captures++;
    if (inside_run) c->n_captures_in_run++;
    return PPDE_OK;
}

// Graph segments of a chains object: PPDE_GRAPH_LEN (one length) or {100, 20}, each only if the histories can hold
// it. Captured and instantiated here, from ppde_chains_init, so that no ppde_chains_run pays for it.
static int capture_segments(ppde_chains* c) {
    if (!c->cfg.use_graph || c->cfg.rng_mode != 1 || !c->graphs.empty()) return PPDE_OK;
    if (c->cfg.which & 4) return PPDE_OK;           // ~900 launches per iteration, tens of milliseconds each way: nothing to gain from replay
    static const int gl_read = env_int("PPDE_GRAPH_LEN", 0), gl_env = gl_read >= 1 && gl_read <= 1000 ? gl_read : 0;
    if (c->recomb.on()) {
        // a segment holds its events at fixed places: its length is a multiple of `every`, and it is replayed from such positions only
        const int every = c->recomb.every;
        std::vector<int> lens;
        if (gl_env) { if (gl_env % every == 0) lens.push_back(gl_env); }
        else if (every <= 100) { lens.push_back(every * (100 / every)); if (lens[0] != every) lens.push_back(every); }
        else if (every <= 1000) lens.push_back(every);
        for (int len : lens) {
            if (len > c->T) continue;
            int rc = capture_segment(c, len, false);
            if (rc) return rc;
        }
        return PPDE_OK;
    }
    const int lens_default[2] = {100, 20};
    for (int k = 0; k < (gl_env ? 1 : 2); ++k) {
        const int len = gl_env ? gl_env : lens_default[k];
        if (len > c->T) continue;
        int rc = capture_segment(c, len, false);
        if (rc) return rc;
    }
    return PPDE_OK;
}

extern "C" {

int ppde_chains_create(ppde_chains** out, ppde_model* m, const ppde_chain_config* cfg) {
    ARGCHK(out && m && cfg, "null argument");
    ARGCHK(cfg->n_chains >= 1, "need at least one chain");
    ARGCHK(cfg->max_steps >= 0, "negative max_steps");
    ARGCHK(cfg->pas_length >= 1 && cfg->pas_length <= 64, "ppde_pas_length out of range");
    ARGCHK(cfg->nmut_threshold >= 0, "negative nmut_threshold");
    ARGCHK(cfg->which >= 1 && cfg->which <= 15 && (cfg->which & 7), "which: bit 0 Potts, bit 1 supervised, bit 2 transformer expert, bit 3 full gradient");
    ARGCHK(!(cfg->which & 4) || m->tf, "transformer expert not set");
    ARGCHK(!(cfg->which & 4) || cfg->n_streams <= 1, "the transformer expert runs on one stream");
    ARGCHK(cfg->min_pos >= 0 && cfg->max_pos < m->L && cfg->min_pos <= cfg->max_pos, "bad [min_pos, max_pos]");
    ARGCHK(cfg->rng_mode == 0 || cfg->rng_mode == 1, "rng_mode must be 0 or 1");
    ARGCHK(cfg->random_chain < cfg->n_chains, "random_chain out of range");
    ARGCHK(!(cfg->which & 1) || m->has_potts, "Potts expert not set");
    ARGCHK(!(cfg->which & 2) || m->has_cnn, "supervised expert not set");
    ARGCHK(cfg->chain_offset + (uint64_t)cfg->n_chains <= 0xffffffffull, "chain_offset + n_chains must fit 32 bits");
    ARGCHK(pas_lds_bytes(m->g) <= 160 * 1024 && m->g.N / 4 <= 3 * PPDE_BLOCK, "sequence too long for the chain kernels (L <= 307)");
    ARGCHK((m->L + 63) / 64 <= PPDE_NW, "more race waves than waves in a chain workgroup");    // (pas.h propose_body_dev: one residue per lane)
    HIPCHK(hipSetDevice(m->device));
    ppde_chains* c = new ppde_chains();
    c->m = m; c->device = m->device; c->cfg = *cfg; c->n = cfg->n_chains; c->T = cfg->max_steps; c->mu_max = 2 * cfg->pas_length - 1;
    const Geom& g = m->g;
    const size_t n = c->n, T1 = (size_t)c->T + 1;
    const int nets = cnn_parts(m);
    bool ok = true;
    auto A = [&](auto** p, size_t count, bool zero) {
        if (!ok) return;
        if (dalloc(p, count) != hipSuccess) { ok = false; return; }
        c->allocs.push_back((void*)*p);
        if (zero && hipMemset((void*)*p, 0, std::max<size_t>(count, 1) * sizeof(**p)) != hipSuccess) ok = false;
    };
    A(&c->cur, n * g.Ls, true); A(&c->prop, n * g.Ls, true);
    c->n_pad = potts_t4_pad(c->n);
    A(&c->curT, g.Lp > 0 ? potts_t4_words(g.NC, c->n_pad) : 1, true); A(&c->propT, g.Lp > 0 ? potts_t4_words(g.NC, c->n_pad) : 1, true);
    A(&c->fb_state, (cfg->paper_results ? n : 1) * g.Ls, true);
    c->rec_stride = chain_rec_stride(c->mu_max);
    A(&c->rec, n * c->rec_stride, true);
    A(&c->grad_cur, cfg->reuse_grad ? n * g.N : 1, true); A(&c->best_state, n * g.L, true); A(&c->rtraj, T1 * g.L, true); A(&c->tmp_acc, n, true);
    A(&c->tmp_idx, n * g.L, true); A(&c->tmp_dist, n, true);
    A(&c->grad, 2 * n * g.N, true); A(&c->epart, 2 * n * std::max(g.Lp, 1), true);
    if (cfg->which & 2) {
        A(&c->gradC, 2 * nets * n * g.N, true); A(&c->fitC, 2 * nets * n, true);
        if (!cnn_single_launch(m)) {
            A(&c->cnn_cmax, cnn_chunk_max_count(m, c->n), true); A(&c->cnn_carg, cnn_chunk_max_count(m, c->n), true);
            A(&c->cnn_cgate, cnn_chunk_gate_count(m, c->n), true);
        }
    }
    if (cfg->which & 4) {
        A(&c->gradT, 2 * n * g.N, true); A(&c->tfE, 2 * n, true);
        if (ok) {
            c->tfw = new TfWork();
            if (tf_alloc_work(m->tf, c->tfw, c->n) != PPDE_OK) ok = false;
        }
    }
    A(&c->fb_grad, (cfg->paper_results ? n : 1) * g.N, true);
    A(&c->fb_e, cfg->paper_results ? n : 1, true); A(&c->fb_f, cfg->paper_results ? n : 1, true);
    A(&c->e_hist, T1 * n, true); A(&c->f_hist, T1 * n, true);
    A(&c->tmp_be, n, true); A(&c->tmp_bf, n, true); A(&c->tmp_bt, n, true);
    A(&c->d_it, 1, true); A(&c->dbg, PPDE_DBG_WORDS, true);
    // error word in pinned host memory mapped into the device: kernels set it with system-scope atomics (error paths
    // only), ppde_chains_sync reads it after the stream has drained, without a device-to-host copy
    if (ok && (hipHostMalloc((void**)&c->h_err, sizeof(int), hipHostMallocMapped) != hipSuccess ||
               hipHostGetDevicePointer((void**)&c->err_flag, c->h_err, 0) != hipSuccess)) ok = false;
    if (ok) *c->h_err = 0;
    if (cfg->trace) {
        A(&c->tr_flat, (size_t)c->T * c->mu_max * n, true); A(&c->tr_acc, (size_t)c->T * n, true);
        A(&c->tr_logacc, (size_t)c->T * n, true); A(&c->tr_U, (size_t)c->T * n, true);
    }
    int K = (cfg->rng_mode == 1 && cfg->n_streams > 1) ? std::min(cfg->n_streams, std::min(8, c->n)) : 1;
    c->streams.assign(K, nullptr);
    c->events.assign(K, nullptr);
    for (int k = 0; k < K && ok; ++k) {
        ok = hipStreamCreateWithFlags(&c->streams[k], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&c->events[k], hipEventDisableTiming) == hipSuccess;
        const int base = c->n / K, extra = c->n % K;
        c->sub_off.push_back(k * base + std::min(k, extra));
        c->sub_n.push_back(base + (k < extra ? 1 : 0));
    }
    if (!ok) {
        delete c;
        return fail(PPDE_ERR_HIP, "device allocation failed while creating chains");
    }
    c->stream = c->streams[0];
    *out = c;
    return PPDE_OK;
}

int ppde_chains_destroy(ppde_chains* c) {
    if (!c) return PPDE_OK;
    hipSetDevice(c->device);
    for (hipStream_t st : c->streams) if (st) hipStreamSynchronize(st);
    delete c;
    return PPDE_OK;
}

int ppde_chains_set_library(ppde_chains* c, const uint32_t* allowed_host) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_library: the library must be set before ppde_chains_init (its graphs hold the pointer)");
    ARGCHK(!c->recomb.on(), "ppde_chains_set_library: recombination is set and holds the open list of the library there was; clear it first "
                            "(ppde_chains_set_recombination(c, NULL))");
    const ppde_model* m = c->m;
    HIPCHK(hipSetDevice(c->device));
    if (!allowed_host) {                            // clear
        c->allowed = {};
        return PPDE_OK;
    }
    int open_in_range = 0;
    for (int l = 0; l < m->L; ++l) {
        const uint32_t w = allowed_host[l];
        if (w >> PPDE_A)
            return fail(PPDE_ERR_INVALID, "design library: residue " + std::to_string(l) + " has a bit >= 20 set (20 letters)");
        if (w && !((w >> m->h_wt[l]) & 1u))          // (the mutation cap's only move is the revert to the wild type)
            return fail(PPDE_ERR_INVALID, "design library: open residue " + std::to_string(l) + " lacks its wild-type letter");
        if (w && l >= c->cfg.min_pos && l <= c->cfg.max_pos) open_in_range++;
    }
    if (!open_in_range)
        return fail(PPDE_ERR_INVALID, "design library: no open residue in [min_pos, max_pos] = [" + std::to_string(c->cfg.min_pos) +
                                      ", " + std::to_string(c->cfg.max_pos) + "]");
    DevBuf<uint32_t> d;
    HIPCHK(d.alloc((size_t)m->L));
    hipError_t e = hipMemcpy(d, allowed_host, (size_t)m->L * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("design library upload: ") + hipGetErrorString(e));
    c->allowed = std::move(d);
    return PPDE_OK;
}

int ppde_chains_set_reversible(ppde_chains* c, int on) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_reversible: the mode must be set before ppde_chains_init (its graphs hold the kernel choice)");
    ARGCHK(!(on && c->cfg.paper_results), "ppde_chains_set_reversible: paper_results restarts a rejected chain from its initial state, "
                                          "which is no Metropolis step; the two cannot be combined");
    ARGCHK(on || !c->temper.on(), "ppde_chains_set_reversible: tempering is set and needs reversible mode (clear it with "
                                  "ppde_chains_set_tempering(c, 0, NULL, 0) first)");
    ARGCHK(on || !c->anneal.on(), "ppde_chains_set_reversible: annealing is set and needs reversible mode (clear it with "
                                  "ppde_chains_set_annealing(c, NULL) first)");
    ARGCHK(on || !c->recomb.on(), "ppde_chains_set_reversible: recombination is set and needs reversible mode (clear it with "
                                  "ppde_chains_set_recombination(c, NULL) first)");
    c->reversible = on != 0;
    return PPDE_OK;
}

int ppde_chains_set_tempering(ppde_chains* c, int n_rungs, const float* beta_host, int swap_every) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_tempering: the ladder must be set before ppde_chains_init (its graphs hold the kernel choice)");
    ARGCHK(!(c->recorder.on() && c->recorder.cfg.rung >= 0), "ppde_chains_set_tempering: a recorder that follows a rung is set; clear it first "
                                                             "(ppde_chains_set_recorder(c, NULL))");
    ARGCHK(!c->stats.on(), "ppde_chains_set_tempering: move statistics are set and were shaped by the ladder there was; clear them first "
                           "(ppde_chains_set_stats(c, NULL))");
    ARGCHK(!c->anneal.on(), "ppde_chains_set_tempering: annealing is set (a schedule and a ladder cannot be combined); clear it first "
                            "(ppde_chains_set_annealing(c, NULL))");
    ARGCHK(!c->recomb.on(), "ppde_chains_set_tempering: recombination is set (its decision takes no beta per chain); clear it first "
                            "(ppde_chains_set_recombination(c, NULL))");
    HIPCHK(hipSetDevice(c->device));
    if (n_rungs == 0 || !beta_host) {               // clear
        c->temper = {};
        return PPDE_OK;
    }
    const int R = n_rungs;
    ARGCHK(c->reversible, "ppde_chains_set_tempering: tempering needs reversible mode (ppde_chains_set_reversible): only there is the "
                          "law at beta, exp(beta E)/Z, defined");
    ARGCHK(R >= 1 && R <= 64, "ppde_chains_set_tempering: n_rungs must be in 1..64");
    for (int r = 0; r < R; ++r) {
        const float b = beta_host[r];
        if (!(b > 0.f) || !(b < INFINITY))
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_tempering: beta[" + std::to_string(r) + "] must be finite and positive");
        if (r > 0 && !(b < beta_host[r - 1]))
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_tempering: the ladder must be strictly decreasing (beta[" + std::to_string(r) +
                                          "] >= beta[" + std::to_string(r - 1) + "])");
    }
    ARGCHK(swap_every >= 0, "ppde_chains_set_tempering: negative swap_every");
    ARGCHK(c->n % R == 0, "ppde_chains_set_tempering: n_chains must be a multiple of n_rungs (ensembles of n_rungs consecutive chains)");
    ARGCHK(c->cfg.chain_offset % (uint64_t)R == 0, "ppde_chains_set_tempering: chain_offset must be a multiple of n_rungs (an ensemble "
                                                   "may not straddle two shards)");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_tempering: n_streams > 1 is not supported (the swap couples "
                                                            "the chains of an ensemble)");
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, pairs = (n / R) * (size_t)(R - 1);
    Tempering t;
    t.n_rungs = R; t.swap_every = swap_every;
    t.ladder.assign(beta_host, beta_host + R);
    hipError_t e = t.beta.alloc(n);
    if (e == hipSuccess) e = t.rung.alloc(n);
    if (e == hipSuccess) e = t.slot.alloc(n);
    if (e == hipSuccess) e = t.swap_attempts.alloc(pairs);
    if (e == hipSuccess) e = t.swap_accepts.alloc(pairs);
    if (e == hipSuccess) e = t.rung_hist.alloc(((size_t)c->T + 1) * n);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_tempering: device allocation: ") + hipGetErrorString(e));
    c->temper = std::move(t);
    return PPDE_OK;
}

int ppde_chains_set_annealing(ppde_chains* c, const ppde_anneal_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_annealing: the schedule must be set before ppde_chains_init (its graphs hold the kernel choice)");
    ARGCHK(!c->recomb.on(), "ppde_chains_set_annealing: recombination is set (its decision takes no beta per chain); clear it first "
                            "(ppde_chains_set_recombination(c, NULL))");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->anneal = {};
        return PPDE_OK;
    }
    ARGCHK(c->reversible, "ppde_chains_set_annealing: annealing needs reversible mode (ppde_chains_set_reversible): only there is the "
                          "law at beta, exp(beta E)/Z, defined");
    ARGCHK(!c->temper.on(), "ppde_chains_set_annealing: tempering is set (a schedule and a ladder cannot be combined); clear it first "
                            "(ppde_chains_set_tempering(c, 0, NULL, 0))");
    ARGCHK(cfg->deme >= 2 && cfg->deme <= ANNEAL_DMAX, "ppde_chains_set_annealing: deme must be in 2..1024");
    ARGCHK(c->n % cfg->deme == 0, "ppde_chains_set_annealing: n_chains must be a multiple of deme (demes of consecutive chains)");
    ARGCHK(c->cfg.chain_offset % (uint64_t)cfg->deme == 0, "ppde_chains_set_annealing: chain_offset must be a multiple of deme (a deme "
                                                           "may not straddle two shards)");
    ARGCHK(cfg->every >= 1, "ppde_chains_set_annealing: every must be >= 1");
    ARGCHK(cfg->n_stages >= 1 && cfg->n_stages <= 4096, "ppde_chains_set_annealing: n_stages must be in 1..4096");
    ARGCHK(cfg->beta, "ppde_chains_set_annealing: no schedule (beta is NULL)");
    const int S = cfg->n_stages, cap = std::min(S, c->T / cfg->every);
    ARGCHK(cap >= 1, "ppde_chains_set_annealing: no event would fit (events_cap = min(n_stages, max_steps / every) is 0)");
    for (int s = 0; s <= S; ++s) {
        const float b = cfg->beta[s];
        if (!(b > 0.f) || !(b < INFINITY))
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_annealing: beta[" + std::to_string(s) + "] must be finite and positive");
        if (s > 0 && b < cfg->beta[s - 1])
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_annealing: the schedule must not decrease (beta[" + std::to_string(s) +
                                          "] < beta[" + std::to_string(s - 1) + "])");
    }
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_annealing: n_streams > 1 is not supported (the selection "
                                                            "couples the chains of a deme)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, demes = n / cfg->deme;
    Annealing t;
    t.D = cfg->deme; t.every = cfg->every; t.S = S; t.cap = cap;
    t.sched.assign(cfg->beta, cfg->beta + S + 1);
    hipError_t e = t.sched_dev.alloc((size_t)S + 1);
    if (e == hipSuccess) e = hipMemcpy(t.sched_dev, cfg->beta, ((size_t)S + 1) * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = t.beta.alloc(n);
    if (e == hipSuccess) e = t.pre.alloc((size_t)cap * n);
    if (e == hipSuccess) e = t.parent.alloc((size_t)cap * n);
    if (e == hipSuccess) e = t.lmw.alloc((size_t)cap * demes);
    if (e == hipSuccess) e = t.ess.alloc((size_t)cap * demes);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_annealing: device allocation: ") + hipGetErrorString(e));
    c->anneal = std::move(t);
    return PPDE_OK;
}

int ppde_chains_set_annealing_adaptive(ppde_chains* c, const ppde_anneal_adaptive_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_annealing_adaptive: the mode must be set before ppde_chains_init (its graphs hold the kernel choice)");
    ARGCHK(!c->recomb.on(), "ppde_chains_set_annealing_adaptive: recombination is set (its decision takes no beta per chain); clear it first "
                            "(ppde_chains_set_recombination(c, NULL))");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->anneal = {};
        return PPDE_OK;
    }
    ARGCHK(c->reversible, "ppde_chains_set_annealing_adaptive: annealing needs reversible mode (ppde_chains_set_reversible): only there is "
                          "the law at beta, exp(beta E)/Z, defined");
    ARGCHK(!c->temper.on(), "ppde_chains_set_annealing_adaptive: tempering is set (a schedule and a ladder cannot be combined); clear it "
                            "first (ppde_chains_set_tempering(c, 0, NULL, 0))");
    ARGCHK(cfg->deme >= 2 && cfg->deme <= ANNEAL_DMAX, "ppde_chains_set_annealing_adaptive: deme must be in 2..1024");
    ARGCHK(c->n % cfg->deme == 0, "ppde_chains_set_annealing_adaptive: n_chains must be a multiple of deme (demes of consecutive chains)");
    ARGCHK(c->cfg.chain_offset % (uint64_t)cfg->deme == 0, "ppde_chains_set_annealing_adaptive: chain_offset must be a multiple of deme (a "
                                                           "deme may not straddle two shards)");
    ARGCHK(cfg->every >= 1, "ppde_chains_set_annealing_adaptive: every must be >= 1");
    ARGCHK(cfg->max_stages >= 1 && cfg->max_stages <= 4096, "ppde_chains_set_annealing_adaptive: max_stages must be in 1..4096");
    const int cap = std::min(cfg->max_stages, c->T / cfg->every);
    ARGCHK(cap >= 1, "ppde_chains_set_annealing_adaptive: no event would fit (events_cap = min(max_stages, max_steps / every) is 0)");
    ARGCHK(cfg->beta_start > 0.f && cfg->beta_start < INFINITY, "ppde_chains_set_annealing_adaptive: beta_start must be finite and positive");
    ARGCHK(cfg->beta_end > 0.f && cfg->beta_end < INFINITY, "ppde_chains_set_annealing_adaptive: beta_end must be finite and positive");
    ARGCHK(cfg->beta_start < cfg->beta_end, "ppde_chains_set_annealing_adaptive: beta_start must be below beta_end");
    ARGCHK(cfg->ess_target > 0.f && cfg->ess_target < 1.f, "ppde_chains_set_annealing_adaptive: ess_target must be inside (0, 1)");
    ARGCHK(cfg->min_step < INFINITY && cfg->min_step >= cfg->beta_end * 0x1p-20f,
           "ppde_chains_set_annealing_adaptive: min_step must be finite and >= beta_end * 2^-20 (a step that changes beta in fp32)");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_annealing_adaptive: n_streams > 1 is not supported (the "
                                                            "selection couples the chains of a deme)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, demes = n / cfg->deme;
    Annealing t;
    t.D = cfg->deme; t.every = cfg->every; t.S = cfg->max_stages; t.cap = cap;
    t.adaptive = true; t.rho = cfg->ess_target; t.min_step = cfg->min_step;
    t.sched = {cfg->beta_start, cfg->beta_end};
    hipError_t e = t.sched_dev.alloc(2);
    if (e == hipSuccess) e = hipMemcpy(t.sched_dev, t.sched.data(), 2 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = t.beta.alloc(n);
    if (e == hipSuccess) e = t.pre.alloc((size_t)cap * n);
    if (e == hipSuccess) e = t.parent.alloc((size_t)cap * n);
    if (e == hipSuccess) e = t.lmw.alloc((size_t)cap * demes);
    if (e == hipSuccess) e = t.ess.alloc((size_t)cap * demes);
    if (e == hipSuccess) e = t.beta_pair.alloc(2 * (size_t)cap * demes);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_annealing_adaptive: device allocation: ") + hipGetErrorString(e));
    c->anneal = std::move(t);
    return PPDE_OK;
}

int ppde_chains_annealing_shape(ppde_chains* c, int32_t* deme, int32_t* events_cap, int32_t* events_done) {
    ARGCHK(c, "null argument");
    ARGCHK(c->anneal.on(), "ppde_chains_annealing_shape: no annealing was set (ppde_chains_set_annealing)");
    if (deme) *deme = c->anneal.D;
    if (events_cap) *events_cap = c->anneal.cap;
    if (events_done) *events_done = c->anneal.events_done(c->steps_done);
    return PPDE_OK;
}

int ppde_chains_annealing_read(ppde_chains* c, int first_event, int n_events, int32_t* parent, float* pre_energy, double* log_mean_w,
                               double* ess, float* beta_now) {
    ARGCHK(c && c->anneal.on(), "ppde_chains_annealing_read: no annealing was set (ppde_chains_set_annealing)");
    ARGCHK(c->initialised, "chains not initialised");
    ARGCHK(first_event >= 0 && n_events >= 0 && first_event + n_events <= c->anneal.events_done(c->steps_done),
           "ppde_chains_annealing_read: events beyond those that have happened (ppde_chains_annealing_shape)");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const size_t n = c->n, demes = n / c->anneal.D, f = (size_t)first_event, k = (size_t)n_events;
    if (parent && k) HIPCHK(hipMemcpy(parent, c->anneal.parent + f * n, k * n * sizeof(int), hipMemcpyDeviceToHost));
    if (pre_energy && k) HIPCHK(hipMemcpy(pre_energy, c->anneal.pre + f * n, k * n * sizeof(float), hipMemcpyDeviceToHost));
    if (log_mean_w && k) HIPCHK(hipMemcpy(log_mean_w, c->anneal.lmw + f * demes, k * demes * sizeof(double), hipMemcpyDeviceToHost));
    if (ess && k) HIPCHK(hipMemcpy(ess, c->anneal.ess + f * demes, k * demes * sizeof(double), hipMemcpyDeviceToHost));
    if (beta_now) HIPCHK(hipMemcpy(beta_now, c->anneal.beta, n * sizeof(float), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_annealing_read_betas(ppde_chains* c, int first_event, int n_events, float* beta_before, float* beta_after) {
    ARGCHK(c && c->anneal.on(), "ppde_chains_annealing_read_betas: no annealing was set (ppde_chains_set_annealing)");
    ARGCHK(c->initialised, "chains not initialised");
    ARGCHK(first_event >= 0 && n_events >= 0 && first_event + n_events <= c->anneal.events_done(c->steps_done),
           "ppde_chains_annealing_read_betas: events beyond those that have happened (ppde_chains_annealing_shape)");
    const Annealing& an = c->anneal;
    const size_t demes = (size_t)c->n / an.D, f = (size_t)first_event, k = (size_t)n_events;
    if (!an.adaptive) {                             // a fixed schedule: every deme walks it
        for (size_t ev = 0; ev < k; ++ev)
            for (size_t d = 0; d < demes; ++d) {
                if (beta_before) beta_before[ev * demes + d] = an.sched[f + ev];
                if (beta_after) beta_after[ev * demes + d] = an.sched[f + ev + 1];
            }
        return PPDE_OK;
    }
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    if (beta_before && k) HIPCHK(hipMemcpy(beta_before, an.beta_pair + f * demes, k * demes * sizeof(float), hipMemcpyDeviceToHost));
    if (beta_after && k)
        HIPCHK(hipMemcpy(beta_after, an.beta_pair + ((size_t)an.cap + f) * demes, k * demes * sizeof(float), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_set_recombination(ppde_chains* c, const ppde_recombine_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_recombination: the mode must be set before ppde_chains_init (its graphs hold the events)");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->recomb = {};
        return PPDE_OK;
    }
    ARGCHK(c->reversible, "ppde_chains_set_recombination: recombination needs reversible mode (ppde_chains_set_reversible): only there "
                          "do the chains have the law exp(E)/Z whose product the exchange keeps");
    ARGCHK(!c->temper.on(), "ppde_chains_set_recombination: tempering is set (the decision takes no beta per chain); clear it first "
                            "(ppde_chains_set_tempering(c, 0, NULL, 0))");
    ARGCHK(!c->anneal.on(), "ppde_chains_set_recombination: annealing is set (the decision takes no beta per chain); clear it first "
                            "(ppde_chains_set_annealing(c, NULL))");
    ARGCHK(!c->cfg.paper_results, "ppde_chains_set_recombination: paper_results is not supported");
    ARGCHK(cfg->deme >= 2 && cfg->deme % 2 == 0, "ppde_chains_set_recombination: deme must be even and >= 2 (the chains of a deme are paired)");
    ARGCHK(c->n % cfg->deme == 0, "ppde_chains_set_recombination: n_chains must be a multiple of deme (demes of consecutive chains)");
    ARGCHK(c->cfg.chain_offset % (uint64_t)cfg->deme == 0, "ppde_chains_set_recombination: chain_offset must be a multiple of deme (a deme "
                                                           "may not straddle two shards)");
    ARGCHK(cfg->every >= 1, "ppde_chains_set_recombination: every must be >= 1");
    const int cap = c->T / cfg->every;
    ARGCHK(cap >= 1, "ppde_chains_set_recombination: no event would fit (events_cap = max_steps / every is 0)");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_recombination: n_streams > 1 is not supported (the exchange "
                                                            "couples the chains of a deme)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const int L = c->m->L;
    std::vector<uint32_t> words;
    if (c->allowed) {
        words.resize((size_t)L);
        HIPCHK(hipMemcpy(words.data(), c->allowed, (size_t)L * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    Recombination t;
    t.D = cfg->deme; t.every = cfg->every; t.cap = cap;
    for (int l = c->cfg.min_pos; l <= c->cfg.max_pos; ++l)
        if (words.empty() || words[(size_t)l]) t.open.push_back(l);
    ARGCHK(!t.open.empty(), "ppde_chains_set_recombination: no open residue in [min_pos, max_pos]");
    const size_t cells = (size_t)cap * c->n;
    hipError_t e = t.open_dev.alloc(t.open.size());
    if (e == hipSuccess) e = hipMemcpy(t.open_dev, t.open.data(), t.open.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = t.partner.alloc(cells);
    if (e == hipSuccess) e = t.lo.alloc(cells);
    if (e == hipSuccess) e = t.hi.alloc(cells);
    if (e == hipSuccess) e = t.differ.alloc(cells);
    if (e == hipSuccess) e = t.child_dist.alloc(cells);
    if (e == hipSuccess) e = t.outcome.alloc(cells);
    if (e == hipSuccess) e = t.log_ratio.alloc(cells);
    if (e == hipSuccess) e = t.pre.alloc(cells);
    if (e == hipSuccess) e = t.child.alloc(cells);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_recombination: device allocation: ") + hipGetErrorString(e));
    c->recomb = std::move(t);
    return PPDE_OK;
}

int ppde_chains_recombination_shape(ppde_chains* c, int32_t* deme, int32_t* n_open, int32_t* open_sites, int32_t* events_cap,
                                    int32_t* events_done) {
    ARGCHK(c, "null argument");
    ARGCHK(c->recomb.on(), "ppde_chains_recombination_shape: no recombination was set (ppde_chains_set_recombination)");
    ARGCHK(c->initialised, "chains not initialised");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    if (deme) *deme = c->recomb.D;
    if (n_open) *n_open = (int32_t)c->recomb.open.size();
    if (open_sites) std::copy(c->recomb.open.begin(), c->recomb.open.end(), open_sites);
    if (events_cap) *events_cap = c->recomb.cap;
    if (events_done) *events_done = c->recomb.events_done(c->steps_done);
    return PPDE_OK;
}

int ppde_chains_recombination_read(ppde_chains* c, int first_event, int n_events, int32_t* partner, int32_t* lo, int32_t* hi,
                                   int32_t* differ, int32_t* child_dist, uint8_t* outcome, float* log_ratio, float* pre_energy,
                                   float* child_energy) {
    ARGCHK(c && c->recomb.on(), "ppde_chains_recombination_read: no recombination was set (ppde_chains_set_recombination)");
    ARGCHK(c->initialised, "chains not initialised");
    ARGCHK(first_event >= 0 && n_events >= 0 && first_event + n_events <= c->recomb.events_done(c->steps_done),
           "ppde_chains_recombination_read: events beyond those that have happened (ppde_chains_recombination_shape)");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const Recombination& r = c->recomb;
    const size_t o = (size_t)first_event * c->n, k = (size_t)n_events * c->n;
    if (!k) return PPDE_OK;
    if (partner) HIPCHK(hipMemcpy(partner, r.partner + o, k * sizeof(int), hipMemcpyDeviceToHost));
    if (lo) HIPCHK(hipMemcpy(lo, r.lo + o, k * sizeof(int), hipMemcpyDeviceToHost));
    if (hi) HIPCHK(hipMemcpy(hi, r.hi + o, k * sizeof(int), hipMemcpyDeviceToHost));
    if (differ) HIPCHK(hipMemcpy(differ, r.differ + o, k * sizeof(int), hipMemcpyDeviceToHost));
    if (child_dist) HIPCHK(hipMemcpy(child_dist, r.child_dist + o, k * sizeof(int), hipMemcpyDeviceToHost));
    if (outcome) HIPCHK(hipMemcpy(outcome, r.outcome + o, k, hipMemcpyDeviceToHost));
    if (log_ratio) HIPCHK(hipMemcpy(log_ratio, r.log_ratio + o, k * sizeof(float), hipMemcpyDeviceToHost));
    if (pre_energy) HIPCHK(hipMemcpy(pre_energy, r.pre + o, k * sizeof(float), hipMemcpyDeviceToHost));
    if (child_energy) HIPCHK(hipMemcpy(child_energy, r.child + o, k * sizeof(float), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

// rungs, temperatures, slots and counters of a fresh start: chain g = chain_offset + b starts on rung g % R (chain_offset % R == 0)
static int init_tempering(ppde_chains* c) {
    const int R = c->temper.n_rungs;
    const size_t n = c->n, pairs = (n / R) * (size_t)(R - 1);
    std::vector<float> hb(n);
    std::vector<int> hr(n), hs(n);
    std::vector<uint8_t> h8(n);
    for (size_t b = 0; b < n; ++b) { hr[b] = (int)(b % R); hb[b] = c->temper.ladder[hr[b]]; hs[b] = (int)b; h8[b] = (uint8_t)hr[b]; }
    HIPCHK(hipMemcpy(c->temper.beta, hb.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->temper.rung, hr.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->temper.slot, hs.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->temper.rung_hist, h8.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->temper.swap_attempts, 0, std::max<size_t>(pairs, 1) * sizeof(long long)));
    HIPCHK(hipMemset(c->temper.swap_accepts, 0, std::max<size_t>(pairs, 1) * sizeof(long long)));
    return PPDE_OK;
}

int ppde_chains_init(ppde_chains* c, const uint8_t* idx0_dev) {
    ARGCHK(c && idx0_dev, "null argument");
    ppde_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    const Geom& g = m->g;
    hipStream_t s = c->stream;
    const int n = c->n;
    hipLaunchKernelGGL(k_pack_state, dim3((n * g.Ls + 255) / 256), dim3(256), 0, s, idx0_dev, c->cur, n, g.L, g.Ls, g.sh);
    HIPCHK(hipGetLastError());
    int rc = state_rows_to_t4(m, c->cur, c->curT, n, c->n_pad, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    *c->h_err = 0;
    HIPCHK(hipMemsetAsync(c->d_it, 0, sizeof(int), s));
    c->d_it_val = 0;
    PasArgs a = chain_args(c);
    if (c->cfg.reuse_grad || c->cfg.paper_results) {
        // fallback rows: the wild type (mutation-cap reset) or the initial population (paper_results)
        const int nf = c->cfg.paper_results ? n : 1;
        const States fstates = c->cfg.paper_results ? cur_states(c) : States{m->d_wt, m->d_wtT, potts_t4_pad(1)};
        if (c->cfg.paper_results) HIPCHK(hipMemcpyAsync(c->fb_state, c->cur, (size_t)n * g.Ls, hipMemcpyDeviceToDevice, s));
        else HIPCHK(hipMemcpyAsync(c->fb_state, m->d_wt, (size_t)g.Ls, hipMemcpyDeviceToDevice, s));
        if (c->cfg.reuse_grad) {
            // evaluate into slot 0 viewed with n = nf (layout [slot][nf][...] only matters within this call)
            EvalTargets t = chain_targets(c, 0);
            rc = eval_experts(m, c->cfg.which, fstates, nf, t, 1, s);
            if (rc) return rc;
            PasArgs f = a;
            f.n = nf;
            hipLaunchKernelGGL(k_combine_rows, dim3(nf), dim3(256), 0, s, f, c->fb_grad);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_slot_energy, dim3((nf + 3) / 4), dim3(256), 0, s, f, c->fb_e, c->fb_f);
            HIPCHK(hipGetLastError());
        }
    } else {
        HIPCHK(hipMemcpyAsync(c->fb_state, m->d_wt, (size_t)g.Ls, hipMemcpyDeviceToDevice, s));
    }
    if (c->cfg.reuse_grad && !c->cfg.paper_results) {   // what a mutation-cap reset continues from
        HIPCHK(hipMemcpyAsync(&c->wt_e, c->fb_e, sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&c->wt_f, c->fb_f, sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        a.wt_e = c->wt_e; a.wt_f = c->wt_f;
    }
    // energies (and, when gradients are reused, the gradient) of the initial population -> slot 0
    rc = eval_experts(m, c->cfg.which, cur_states(c), n, chain_targets(c, 0), 1, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_init_chain, dim3((n + 3) / 4), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    if (c->cfg.reuse_grad) {   // the current state's combined gradient row travels with the chain from here on
        hipLaunchKernelGGL(k_combine_rows, dim3(n), dim3(256), 0, s, a, c->grad_cur);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    if (c->temper.on()) {
        rc = init_tempering(c);
        if (rc) return rc;
    }
    if (c->anneal.on()) {                                 // (a fresh start: every chain at beta[0])
        const std::vector<float> hb((size_t)n, c->anneal.sched[0]);
        HIPCHK(hipMemcpy(c->anneal.beta, hb.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    }
    if (c->recorder.on()) HIPCHK(hipMemset(c->recorder.counts, 0, (size_t)g.L * PPDE_A * sizeof(unsigned long long)));   // (a fresh start counts from zero)
    if (c->pairs.on()) HIPCHK(hipMemset(c->pairs.counts, 0, c->pairs.tiles() * PAIR_TILE * sizeof(unsigned long long)));
    if (c->archive.on()) {                              // (a fresh start: an empty archive, then the initial population as t = 0)
        HIPCHK(hipMemsetAsync(c->archive.count, 0, (size_t)n * sizeof(int), s));
        rc = launch_archive(c, nullptr, -1, s);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(s));
    }
    if (c->stats.on()) {                               // (a fresh start: zero counters, the initial population as the state before iteration 0)
        HIPCHK(hipMemsetAsync(c->stats.cnt, 0, c->stats.cells_total() * sizeof(long long), s));
        HIPCHK(hipMemcpyAsync(c->stats.prev, c->cur, (size_t)n * g.Ls, hipMemcpyDeviceToDevice, s));   // (buffer 0: iteration 0 reads it)
        hipLaunchKernelGGL(k_stats_init, dim3((n + 255) / 256), dim3(256), 0, s, c->rec, c->rec_stride, c->stats.dist, n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    c->steps_done = 0;
    c->initialised = true;
    rc = capture_segments(c);                       // (replayed by every later run; never captured inside one)
    if (rc) return rc;
    return PPDE_OK;
}

int ppde_chains_run(ppde_chains* c, int steps, const int32_t* U_dev, const float* q_dev, const float* u_dev,
                    const int32_t* max_u) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(steps >= 0 && c->steps_done + steps <= c->T, "run would exceed max_steps");
    ppde_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    const Geom& g = m->g;
    if (c->cfg.rng_mode == 0) {
        ARGCHK(steps == 0 || (U_dev && q_dev && u_dev && max_u), "rng_mode 0 needs U, q, u and max_u");
        size_t qoff = 0;
        for (int i = 0; i < steps; ++i) {
            ARGCHK(max_u[i] >= 1 && max_u[i] <= c->mu_max, "max_u out of range");
            int rc = enqueue_iterations(c, 0, nullptr, c->steps_done + i, 1, U_dev + (size_t)i * c->n,
                                        q_dev + qoff * c->n * g.N, u_dev + (size_t)i * c->n, max_u[i]);
            if (rc) return rc;
            qoff += max_u[i];
        }
        c->steps_done += steps;
        return PPDE_OK;
    }
    int done = 0;
    if (c->recomb.on() && !c->graphs.empty()) {
        // segments start at multiples of `every` only: eager iterations up to the next such position, then the longest segment that
        // fits, and the rest eagerly
        const int every = c->recomb.every;
        while (done < steps) {
            const int pos = c->steps_done + done, left = steps - done;
            const ppde_chains::GraphSeg* seg = nullptr;
            if (pos % every == 0)
                for (const auto& gs : c->graphs) if (gs.len <= left) { seg = &gs; break; }       // longest first
            if (seg) {
                if (c->d_it_val != (long long)pos) {
                    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->d_it, pos, 1, c->stream));
                    c->d_it_val = (long long)pos;
                }
                HIPCHK(hipGraphLaunch(seg->exec, c->stream));
                done += seg->len;
                c->d_it_val += seg->len;
                c->n_replayed_steps += seg->len;
                continue;
            }
            const int k = pos % every == 0 ? left : std::min(left, every - pos % every);
            int rc = enqueue_block(c, nullptr, pos, k);
            if (rc) return rc;
            c->n_eager_steps += k;
            done += k;
        }
        c->steps_done += steps;
        return PPDE_OK;
    }
    if (!c->graphs.empty()) {
        for (const auto& gs : c->graphs) {          // longest segment first
            while (steps - done >= gs.len) {
                // every segment ends by adding its length to the device counter: it only needs setting after eager
                // iterations (which take their index from the launch arguments and leave the counter behind)
                if (c->d_it_val != (long long)c->steps_done + done) {
                    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->d_it, c->steps_done + done, 1, c->stream));
                    c->d_it_val = (long long)c->steps_done + done;
                }
                HIPCHK(hipGraphLaunch(gs.exec, c->stream));
                done += gs.len;
                c->d_it_val += gs.len;
            }
        }
        c->n_replayed_steps += done;
    }
    if (done < steps) {
        int rc = enqueue_block(c, nullptr, c->steps_done + done, steps - done);
        if (rc) return rc;
        c->n_eager_steps += steps - done;
    }
    c->steps_done += steps;
    return PPDE_OK;
}

int ppde_chains_graph_stats(ppde_chains* c, int32_t* captures, int32_t* captures_in_run, int64_t* replayed_steps,
                            int64_t* eager_steps) {
    ARGCHK(c, "null chains");
    if (captures) *captures = c->n_captures;
    if (captures_in_run) *captures_in_run = c->n_captures_in_run;
    if (replayed_steps) *replayed_steps = c->n_replayed_steps;
    if (eager_steps) *eager_steps = c->n_eager_steps;
    return PPDE_OK;
}

int ppde_chains_sync(ppde_chains* c) {
    ARGCHK(c, "null chains");
    HIPCHK(hipSetDevice(c->m->device));
    // short runs are latency-bound on the host side too: poll the stream for a while before blocking in the driver
    // (a blocking wait wakes up tens of microseconds after the last kernel; a 20-iteration block is 500 us)
    hipError_t q = hipErrorNotReady;
    for (int spin = 0; spin < 20000 && (q = hipStreamQuery(c->stream)) == hipErrorNotReady; ++spin) { }
    if (q == hipErrorNotReady) q = hipStreamSynchronize(c->stream);
    HIPCHK(q);
    const int err = *(volatile int*)c->h_err;
    if (err & 2) return fail(PPDE_ERR_INVALID, "a supplied path length U exceeds the max_u of its iteration (the noise block holds only max_u sub-steps)");
    if (err) return fail(PPDE_ERR_NUMERIC, "a proposal row had no usable mass (every move masked out, or every admissible logit 86.6 or more below / one 88.7 above the softmax reference): the categorical is undefined");
    return PPDE_OK;
}

int ppde_chains_steps_done(ppde_chains* c) { return c ? c->steps_done : PPDE_ERR_INVALID; }

// `units` x `per_unit` state rows [Ls] at the device address `src` -> plain rows [L] at the host address `dst`, through a device
// buffer, a block of whole units at a time (32-bit thread indices: at most 2^30 per launch)
static int read_state_rows(ppde_chains* c, const uint8_t* src, size_t units, size_t per_unit, uint8_t* dst) {
    const Geom& g = c->m->g;
    const size_t L = g.L, per = per_unit * (size_t)std::max(g.L, g.Ls);
    const size_t block = std::max<size_t>(1, std::min<size_t>(units, ((size_t)1 << 30) / per));
    DevBuf<uint8_t> tmp;
    HIPCHK(tmp.alloc(block * per_unit * L));
    for (size_t u = 0; u < units; u += block) {
        const int rows_n = (int)(std::min(block, units - u) * per_unit);
        hipLaunchKernelGGL(k_unpack_state, dim3((rows_n * g.L + 255) / 256), dim3(256), 0, c->stream,
                           src + u * per_unit * g.Ls, tmp.p, rows_n, g.L, g.Ls, g.sh);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(dst + u * per_unit * L, tmp.p, (size_t)rows_n * L, hipMemcpyDeviceToHost));
    }
    return PPDE_OK;
}

int ppde_chains_peek(ppde_chains* c, uint8_t* idx, float* energy, float* fitness, uint8_t* accepted, int32_t* dist) {
    ARGCHK(c && c->initialised, "chains not initialised");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const Geom& g = c->m->g;
    const int n = c->n;
    hipStream_t s = c->stream;
    if (idx) {
        hipLaunchKernelGGL(k_unpack_state, dim3((n * g.L + 255) / 256), dim3(256), 0, s, c->cur, c->tmp_idx, n, g.L, g.Ls, g.sh);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(idx, c->tmp_idx, (size_t)n * g.L, hipMemcpyDeviceToHost, s));
    }
    if (dist) {
        hipLaunchKernelGGL(k_mut_distance, dim3((n + 3) / 4), dim3(256), 0, s, c->cur, c->m->d_wt, n, g.L, g.Ls, g.sh, c->tmp_dist);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dist, c->tmp_dist, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (energy) HIPCHK(hipMemcpyAsync(energy, c->e_hist + (size_t)c->steps_done * n, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (fitness) HIPCHK(hipMemcpyAsync(fitness, c->f_hist + (size_t)c->steps_done * n, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (accepted) {
        hipLaunchKernelGGL(k_rec_gather, dim3((n + 255) / 256), dim3(256), 0, s, chain_args(c), (float*)nullptr, (float*)nullptr,
                           (int*)nullptr, c->tmp_acc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(accepted, c->tmp_acc, n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return PPDE_OK;
}

int ppde_chains_collect(ppde_chains* c, uint8_t* best_idx, float* best_energy, float* best_fitness, int32_t* best_step,
                        float* energy_history, float* fitness_history, uint8_t* random_traj) {
    ARGCHK(c && c->initialised, "chains not initialised");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const Geom& g = c->m->g;
    const size_t n = c->n, rows = (size_t)c->steps_done + 1;
    if (best_idx) HIPCHK(hipMemcpy(best_idx, c->best_state, n * g.L, hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(k_rec_gather, dim3(((int)n + 255) / 256), dim3(256), 0, c->stream, chain_args(c), c->tmp_be, c->tmp_bf,
                       c->tmp_bt, (uint8_t*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    if (best_energy) HIPCHK(hipMemcpy(best_energy, c->tmp_be, n * sizeof(float), hipMemcpyDeviceToHost));
    if (best_fitness) HIPCHK(hipMemcpy(best_fitness, c->tmp_bf, n * sizeof(float), hipMemcpyDeviceToHost));
    if (best_step) HIPCHK(hipMemcpy(best_step, c->tmp_bt, n * sizeof(int), hipMemcpyDeviceToHost));
    if (energy_history) HIPCHK(hipMemcpy(energy_history, c->e_hist, rows * n * sizeof(float), hipMemcpyDeviceToHost));
    if (fitness_history) HIPCHK(hipMemcpy(fitness_history, c->f_hist, rows * n * sizeof(float), hipMemcpyDeviceToHost));
    if (random_traj) {
        ARGCHK(c->cfg.random_chain >= 0, "no random trajectory was recorded (random_chain = -1)");
        HIPCHK(hipMemcpy(random_traj, c->rtraj, rows * g.L, hipMemcpyDeviceToHost));
    }
    return PPDE_OK;
}

int ppde_chains_tempering_state(ppde_chains* c, int32_t* rung, float* beta, int64_t* swap_attempts, int64_t* swap_accepts) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(c->temper.on(), "ppde_chains_tempering_state: no tempering was set (ppde_chains_set_tempering)");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const size_t n = c->n, pairs = (n / c->temper.n_rungs) * (size_t)(c->temper.n_rungs - 1);
    if (rung) HIPCHK(hipMemcpy(rung, c->temper.rung, n * sizeof(int), hipMemcpyDeviceToHost));
    if (beta) HIPCHK(hipMemcpy(beta, c->temper.beta, n * sizeof(float), hipMemcpyDeviceToHost));
    if (swap_attempts && pairs) HIPCHK(hipMemcpy(swap_attempts, c->temper.swap_attempts, pairs * sizeof(long long), hipMemcpyDeviceToHost));
    if (swap_accepts && pairs) HIPCHK(hipMemcpy(swap_accepts, c->temper.swap_accepts, pairs * sizeof(long long), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_tempering_history(ppde_chains* c, uint8_t* rung_history) {
    ARGCHK(c && c->initialised && rung_history, "chains not initialised, or null argument");
    ARGCHK(c->temper.on(), "ppde_chains_tempering_history: no tempering was set (ppde_chains_set_tempering)");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    HIPCHK(hipMemcpy(rung_history, c->temper.rung_hist, ((size_t)c->steps_done + 1) * c->n, hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_set_recorder(ppde_chains* c, const ppde_record_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_recorder: the recorder must be set before ppde_chains_init (its graphs hold the pointers)");
    ARGCHK(!c->pairs.on(), "ppde_chains_set_recorder: pair counts are set and follow this recorder's schedule; clear the pair counts first "
                           "(ppde_chains_set_pair_counts(c, NULL))");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->recorder = {};
        return PPDE_OK;
    }
    ARGCHK(cfg->every >= 1, "ppde_chains_set_recorder: every must be >= 1");
    ARGCHK(cfg->burn_in >= 0, "ppde_chains_set_recorder: negative burn_in");
    ARGCHK(cfg->rung >= -1, "ppde_chains_set_recorder: rung must be -1 (every chain) or a rung of the ladder");
    ARGCHK(cfg->keep_samples == 0 || cfg->keep_samples == 1, "ppde_chains_set_recorder: keep_samples must be 0 or 1");
    ARGCHK(cfg->rung < 0 || c->temper.on(), "ppde_chains_set_recorder: following a rung needs tempering (ppde_chains_set_tempering first)");
    ARGCHK(cfg->rung < c->temper.n_rungs || cfg->rung < 0, "ppde_chains_set_recorder: rung beyond the ladder");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_recorder: n_streams > 1 is not supported (the counters have one "
                                                            "owner per launch)");
    const int rows_cap = c->T > cfg->burn_in ? (c->T - cfg->burn_in) / cfg->every : 0;
    ARGCHK(rows_cap >= 1, "ppde_chains_set_recorder: no iteration of max_steps would be recorded (burn_in + every > max_steps)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const Geom& g = c->m->g;
    const size_t slots = cfg->rung >= 0 ? (size_t)c->n / c->temper.n_rungs : (size_t)c->n, cells = (size_t)rows_cap * slots;
    const size_t n_counts = (size_t)g.L * PPDE_A;
    Recorder t;
    t.cfg = *cfg; t.rows_cap = rows_cap; t.slots = (int)slots;
    hipError_t e = t.counts.alloc_zero(n_counts);
    if (cfg->keep_samples) {
        if (e == hipSuccess) e = t.idx.alloc_zero(cells * (size_t)g.Ls);
        if (e == hipSuccess) e = t.e.alloc(cells);
        if (e == hipSuccess) e = t.f.alloc(cells);
        if (e == hipSuccess) e = t.chain.alloc(cells);
    }
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_recorder: device allocation: ") + hipGetErrorString(e));
    c->recorder = std::move(t);
    return PPDE_OK;
}

int ppde_chains_recorder_shape(ppde_chains* c, int32_t* rows_done, int32_t* rows_cap, int32_t* slots) {
    ARGCHK(c, "null argument");
    ARGCHK(c->recorder.on(), "ppde_chains_recorder_shape: no recorder was set (ppde_chains_set_recorder)");
    if (rows_done) *rows_done = c->initialised ? c->recorder.rows_done(c->steps_done) : 0;
    if (rows_cap) *rows_cap = c->recorder.rows_cap;
    if (slots) *slots = c->recorder.slots;
    return PPDE_OK;
}

int ppde_chains_recorder_read(ppde_chains* c, int first_row, int n_rows, uint8_t* idx, float* energy, float* fitness,
                              int32_t* chain, uint64_t* site_counts) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(c->recorder.on(), "ppde_chains_recorder_read: no recorder was set (ppde_chains_set_recorder)");
    ARGCHK(first_row >= 0 && n_rows >= 0 && (long long)first_row + n_rows <= c->recorder.rows_done(c->steps_done),
           "ppde_chains_recorder_read: rows beyond those recorded so far (ppde_chains_recorder_shape: rows_done)");
    ARGCHK(c->recorder.cfg.keep_samples || !(idx || energy || fitness || chain),
           "ppde_chains_recorder_read: the recorder keeps site counts only (keep_samples = 0): pass NULL for the samples");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const Geom& g = c->m->g;
    const size_t slots = c->recorder.slots, cells = (size_t)n_rows * slots, o = (size_t)first_row * slots;
    if (idx && cells && (rc = read_state_rows(c, c->recorder.idx + o * g.Ls, (size_t)n_rows, slots, idx))) return rc;   // [rows][slots][Ls] -> [L]
    if (energy && cells) HIPCHK(hipMemcpy(energy, c->recorder.e + o, cells * sizeof(float), hipMemcpyDeviceToHost));
    if (fitness && cells) HIPCHK(hipMemcpy(fitness, c->recorder.f + o, cells * sizeof(float), hipMemcpyDeviceToHost));
    if (chain && cells) HIPCHK(hipMemcpy(chain, c->recorder.chain + o, cells * sizeof(int), hipMemcpyDeviceToHost));
    if (site_counts) HIPCHK(hipMemcpy(site_counts, c->recorder.counts, (size_t)g.L * PPDE_A * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_set_archive(ppde_chains* c, const ppde_archive_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_archive: the archive must be set before ppde_chains_init (its graphs hold the pointers)");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->archive = {};
        return PPDE_OK;
    }
    ARGCHK(cfg->k >= 1 && cfg->k <= ARCH_KMAX, "ppde_chains_set_archive: k must be in 1..32");
    ARGCHK(!c->cfg.paper_results, "ppde_chains_set_archive: paper_results is not supported (after a rejection its history row holds the "
                                  "energy of the state that was left while the chain continues from its initial state: a mismatched pair)");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_archive: n_streams > 1 is not supported (one launch archives "
                                                            "every chain of the object)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const Geom& g = c->m->g;
    const size_t n = c->n, cells = n * (size_t)cfg->k;
    Archive t;
    t.k = cfg->k;
    hipError_t e = t.idx.alloc_zero(cells * (size_t)g.Ls);
    if (e == hipSuccess) e = t.e.alloc(cells);
    if (e == hipSuccess) e = t.f.alloc(cells);
    if (e == hipSuccess) e = t.step.alloc(cells);
    if (e == hipSuccess) e = t.hash.alloc(cells);
    if (e == hipSuccess) e = t.count.alloc_zero(n);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_archive: device allocation: ") + hipGetErrorString(e));
    c->archive = std::move(t);
    return PPDE_OK;
}

int ppde_chains_archive_shape(ppde_chains* c, int32_t* k) {
    ARGCHK(c, "null argument");
    ARGCHK(c->archive.on(), "ppde_chains_archive_shape: no archive was set (ppde_chains_set_archive)");
    if (k) *k = c->archive.k;
    return PPDE_OK;
}

int ppde_chains_archive_read(ppde_chains* c, uint8_t* idx, float* energy, float* fitness, int32_t* step, int32_t* count) {
    ARGCHK(c && c->archive.on(), "ppde_chains_archive_read: no archive was set (ppde_chains_set_archive)");
    ARGCHK(c->initialised, "chains not initialised");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const Geom& g = c->m->g;
    const size_t n = c->n, K = c->archive.k, cells = n * K, L = g.L;
    std::vector<float> he(cells), hf(cells);
    std::vector<int> hs(cells), hc(n);
    HIPCHK(hipMemcpy(he.data(), c->archive.e, cells * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hf.data(), c->archive.f, cells * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hs.data(), c->archive.step, cells * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hc.data(), c->archive.count, n * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<uint8_t> hi;
    if (idx) {
        hi.resize(cells * L);
        if ((rc = read_state_rows(c, c->archive.idx, n, K, hi.data()))) return rc;   // [n][K][Ls] -> [n][K][L]
    }
    // each chain's entries by (energy descending, step ascending); the slots beyond count filled
    std::vector<int> order(K);
    for (size_t b = 0; b < n; ++b) {
        const int cnt = std::max(0, std::min(hc[b], (int)K));
        const size_t o = b * K;
        for (int j = 0; j < cnt; ++j) order[j] = j;
        std::sort(order.begin(), order.begin() + cnt, [&](int x, int y) {
            return he[o + x] > he[o + y] || (he[o + x] == he[o + y] && hs[o + x] < hs[o + y]);
        });
        for (size_t j = 0; j < K; ++j) {
            const bool live = (int)j < cnt;
            const size_t src = o + (live ? order[j] : 0);
            if (energy) energy[o + j] = live ? he[src] : -INFINITY;
            if (fitness) fitness[o + j] = live ? hf[src] : 0.f;
            if (step) step[o + j] = live ? hs[src] : -1;
            if (idx) {
                if (live) memcpy(idx + (o + j) * L, hi.data() + src * L, L);
                else memset(idx + (o + j) * L, 255, L);
            }
        }
        if (count) count[b] = cnt;
    }
    return PPDE_OK;
}

int ppde_chains_set_stats(ppde_chains* c, const ppde_stats_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_stats: the statistics must be set before ppde_chains_init (its graphs hold the pointers)");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->stats = {};
        return PPDE_OK;
    }
    ARGCHK(cfg->per_site == 0 || cfg->per_site == 1, "ppde_chains_set_stats: per_site must be 0 or 1");
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, "ppde_chains_set_stats: n_streams > 1 is not supported (the counters have one "
                                                            "owner per launch)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const Geom& g = c->m->g;
    MoveStats t;
    t.n = c->n; t.R = std::max(c->temper.n_rungs, 1); t.M = c->mu_max; t.L = g.L; t.per_site = cfg->per_site;
    hipError_t e = t.cnt.alloc_zero(t.cells_total());
    if (e == hipSuccess) e = t.prev.alloc_zero(2 * (size_t)t.n * g.Ls);
    if (e == hipSuccess) e = t.dist.alloc_zero((size_t)t.n);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_stats: device allocation: ") + hipGetErrorString(e));
    c->stats = std::move(t);
    return PPDE_OK;
}

int ppde_chains_stats_shape(ppde_chains* c, int32_t* n_rungs, int32_t* n_lengths, int32_t* per_site) {
    ARGCHK(c, "null argument");
    ARGCHK(c->stats.on(), "ppde_chains_stats_shape: no statistics were set (ppde_chains_set_stats)");
    if (n_rungs) *n_rungs = c->stats.R;
    if (n_lengths) *n_lengths = c->mu_max;
    if (per_site) *per_site = c->stats.per_site;
    return PPDE_OK;
}

int ppde_chains_stats_read(ppde_chains* c, int64_t* iters, int64_t* accepts, int64_t* moved, int64_t* jump_sum, int64_t* dist_sum,
                           int64_t* wt_returns, int64_t* len_attempts, int64_t* len_accepts, int64_t* site_changes) {
    ARGCHK(c && c->stats.on(), "ppde_chains_stats_read: no statistics were set (ppde_chains_set_stats)");
    ARGCHK(c->initialised, "chains not initialised");
    ARGCHK(c->stats.per_site || !site_changes, "ppde_chains_stats_read: the statistics keep no per-site counts (per_site = 0): pass NULL "
                                               "for site_changes");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    int64_t* out[9] = {iters, accepts, moved, jump_sum, dist_sum, wt_returns, len_attempts, len_accepts, site_changes};
    for (int k = 0; k < 9; ++k)
        if (out[k] && c->stats.cells(k))
            HIPCHK(hipMemcpy(out[k], c->stats.counter(k), c->stats.cells(k) * sizeof(long long), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_set_pair_counts(ppde_chains* c, const ppde_pair_config* cfg) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, "ppde_chains_set_pair_counts: pair counts must be set before ppde_chains_init (its graphs hold the pointers)");
    if (!cfg) {                                     // clear
        HIPCHK(hipSetDevice(c->device));
        c->pairs = {};
        return PPDE_OK;
    }
    ARGCHK(c->recorder.on(), "ppde_chains_set_pair_counts: no recorder was set (pair counts follow its schedule and slots: "
                             "ppde_chains_set_recorder first)");
    const int L = c->m->g.L;
    ARGCHK(cfg->n_sites >= 0 && cfg->n_sites <= L, "ppde_chains_set_pair_counts: n_sites must be in 0..L (0: every residue)");
    ARGCHK(cfg->n_sites == 0 || cfg->sites, "ppde_chains_set_pair_counts: n_sites > 0 needs a site list");
    ARGCHK(cfg->n_sites > 0 || !cfg->sites, "ppde_chains_set_pair_counts: a site list with n_sites = 0 (0 with NULL selects every residue)");
    const int S = cfg->n_sites ? cfg->n_sites : L;
    for (int i = 0; i < cfg->n_sites; ++i) {
        if (cfg->sites[i] < 0 || cfg->sites[i] >= L)
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_pair_counts: sites[" + std::to_string(i) + "] = " + std::to_string(cfg->sites[i]) +
                                          " lies outside the sequence 0.." + std::to_string(L - 1));
        if (i > 0 && cfg->sites[i] <= cfg->sites[i - 1])
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_pair_counts: the sites must be strictly increasing (sites[" + std::to_string(i) +
                                          "] <= sites[" + std::to_string(i - 1) + "])");
    }
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    PairCounts t;
    t.nt = (S + PAIR_TS - 1) / PAIR_TS;
    std::vector<int32_t> padded((size_t)t.nt * PAIR_TS, -1);
    for (int i = 0; i < S; ++i) padded[i] = cfg->n_sites ? cfg->sites[i] : i;
    t.sites.assign(padded.begin(), padded.begin() + S);
    hipError_t e = t.sites_dev.alloc(padded.size());
    if (e == hipSuccess) e = hipMemcpy(t.sites_dev, padded.data(), padded.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = t.counts.alloc_zero(t.tiles() * PAIR_TILE);
    if (e != hipSuccess) return fail(PPDE_ERR_HIP, std::string("ppde_chains_set_pair_counts: device allocation: ") + hipGetErrorString(e));
    c->pairs = std::move(t);
    return PPDE_OK;
}

int ppde_chains_pair_counts_shape(ppde_chains* c, int32_t* n_sites, int32_t* sites) {
    ARGCHK(c, "null argument");
    ARGCHK(c->pairs.on(), "ppde_chains_pair_counts_shape: no pair counts were set (ppde_chains_set_pair_counts)");
    if (n_sites) *n_sites = (int32_t)c->pairs.sites.size();
    if (sites) std::copy(c->pairs.sites.begin(), c->pairs.sites.end(), sites);
    return PPDE_OK;
}

int ppde_chains_pair_counts_read(ppde_chains* c, uint64_t* pair_counts) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(c->pairs.on(), "ppde_chains_pair_counts_read: no pair counts were set (ppde_chains_set_pair_counts)");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    if (!pair_counts) return PPDE_OK;
    // the device keeps the upper block triangle, tile by tile (pairs.h): one row of tiles at a time to the host, mirrored here
    const size_t S = c->pairs.sites.size(), W = S * PPDE_A;
    const int nt = c->pairs.nt;
    std::vector<unsigned long long> rowbuf((size_t)nt * PAIR_TILE);
    size_t first = 0;
    for (int ti = 0; ti < nt; ++ti) {
        const size_t tiles = (size_t)(nt - ti);
        HIPCHK(hipMemcpy(rowbuf.data(), c->pairs.counts + first * PAIR_TILE, tiles * PAIR_TILE * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
        first += tiles;
        for (int tj = ti; tj < nt; ++tj)
            for (int p = 0; p < PAIR_TS; ++p)
                for (int q = 0; q < PAIR_TS; ++q) {
                    const size_t i = (size_t)ti * PAIR_TS + p, j = (size_t)tj * PAIR_TS + q;
                    if (i >= S || j >= S) continue;
                    const unsigned long long* bins = rowbuf.data() + ((size_t)(tj - ti) * PAIR_TS * PAIR_TS + p * PAIR_TS + q) * PAIR_BINS;
                    for (int x = 0; x < PPDE_A; ++x)
                        for (int y = 0; y < PPDE_A; ++y) {
                            const uint64_t v = bins[x * PPDE_A + y];
                            pair_counts[(i * PPDE_A + x) * W + j * PPDE_A + y] = v;
                            if (tj != ti) pair_counts[(j * PPDE_A + y) * W + i * PPDE_A + x] = v;
                        }
                }
    }
    return PPDE_OK;
}

int ppde_chains_trace(ppde_chains* c, int32_t* flat, uint8_t* accepted, float* log_acc, int32_t* U) {
    ARGCHK(c && c->cfg.trace, "chains were created without trace");
    int rc = ppde_chains_sync(c);
    if (rc) return rc;
    const size_t n = c->n, t = c->steps_done;
    if (flat) HIPCHK(hipMemcpy(flat, c->tr_flat, t * c->mu_max * n * sizeof(int), hipMemcpyDeviceToHost));
    if (accepted) HIPCHK(hipMemcpy(accepted, c->tr_acc, t * n, hipMemcpyDeviceToHost));
    if (log_acc) HIPCHK(hipMemcpy(log_acc, c->tr_logacc, t * n * sizeof(float), hipMemcpyDeviceToHost));
    if (U) HIPCHK(hipMemcpy(U, c->tr_U, t * n * sizeof(int), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

int ppde_chains_philox_dump(ppde_chains* c, int it, int s, float* q_dev, float* u_dev, int32_t* U_dev) {
    ARGCHK(c && q_dev && u_dev && U_dev, "null argument");
    ARGCHK(s >= 0 && s < c->mu_max, "sub-step out of range");
    HIPCHK(hipSetDevice(c->m->device));
    PasArgs a = chain_args(c);
    hipLaunchKernelGGL(k_philox_dump, dim3(c->n), dim3(256), 0, c->stream, a.key, it, s, c->cfg.pas_length, c->n,
                       c->m->g.N, q_dev, u_dev, U_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return PPDE_OK;
}

#ifdef PPDE_STAMPS
int ppde_debug_read_stamps(ppde_chains* c, unsigned long long* out128) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out128, c->dbg, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PPDE_OK;
}
// per-workgroup records of the last k_cnn launch: [wg][4] = 100 MHz ticks at entry, route start, route end, exit
int ppde_debug_read_wg_stamps(ppde_chains* c, unsigned long long* out, int words) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->dbg + 128, (size_t)std::min(words, PPDE_DBG_WORDS - 128) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PPDE_OK;
}
#endif

int ppde_chains_time_potts_in_situ(ppde_chains* c, int iters, float* avg_us, int* launches, float* avg_dispatch_us) {
    ARGCHK(c && c->initialised && avg_us && launches && iters >= 1, "bad argument");
    // only launch_potts and launch_chain_kernel bind events: with another expert in the energy the event in front of a Potts
    // launch would not be its immediate predecessor's
    ARGCHK((c->cfg.which & 7) == 1, "in-situ timing is defined for the Potts-only energy (which = 1)");
    ARGCHK(c->cfg.rng_mode == 1, "in-situ timing needs the device RNG");
    ARGCHK(c->steps_done + iters <= c->T, "run would exceed max_steps");
    ARGCHK(c->streams.size() == 1, "in-situ timing takes consecutive dispatches of ONE stream");
    HIPCHK(hipSetDevice(c->m->device));
    EventPool pool;
    pool.ev.assign((size_t)iters * 4 * c->streams.size() + 4, nullptr);     // every kernel of an iteration: <= 2 expert + 2 chain launches
    pool.is_potts.assign(pool.ev.size(), 0);
    for (auto& e : pool.ev) HIPCHK(hipEventCreate(&e));
    g_potts_events = &pool;
    int rc = enqueue_block(c, nullptr, c->steps_done, iters);
    g_potts_events = nullptr;
    if (rc == PPDE_OK) {
        c->steps_done += iters;
        rc = ppde_chains_sync(c);
    }
    if (rc) return rc;
    ARGCHK(!pool.exhausted, "event pool exhausted: a launch went out untimed");
    double tot = 0.0, tot_d = 0.0;
    int cnt = 0, cnt_d = 0;
    for (size_t i = 1; i < pool.used; ++i) {                             // predecessor's end -> this Potts launch's end
        float ms = 0.f;
        if (!pool.is_potts[i]) continue;
        if (hipEventElapsedTime(&ms, pool.ev[i - 1], pool.ev[i]) == hipSuccess) { tot += ms; ++cnt; }
        // the dispatch's own interval: an event bound to a kernel against itself yields that command's start -> end as the
        // command processor stamped them (the pair rocprofv3's kernel trace reads)
        if (hipEventElapsedTime(&ms, pool.ev[i], pool.ev[i]) == hipSuccess) { tot_d += ms; ++cnt_d; }
    }
    (void)hipGetLastError();
    ARGCHK(cnt > 0, "no Potts launch was timed");
    *avg_us = (float)(tot * 1000.0 / cnt);
    *launches = cnt;
    if (avg_dispatch_us) *avg_dispatch_us = cnt_d ? (float)(tot_d * 1000.0 / cnt_d) : 0.f;
    return PPDE_OK;
}

int ppde_chains_time_experts(ppde_chains* c, int reps, float* avg_us) {
    ARGCHK(c && c->initialised && avg_us && reps >= 1, "bad argument");
    HIPCHK(hipSetDevice(c->m->device));
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    // current states into the proposal slot, exactly as the evaluation inside an iteration launches it
    int rc = eval_experts(c->m, c->cfg.which, cur_states(c), c->n, chain_targets(c, 1), 1, c->stream);   // warm
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev.a, c->stream));
    for (int i = 0; i < reps; ++i)
        if ((rc = eval_experts(c->m, c->cfg.which, cur_states(c), c->n, chain_targets(c, 1), 1, c->stream))) return rc;
    HIPCHK(hipEventRecord(ev.b, c->stream));
    HIPCHK(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.f / reps;
    return PPDE_OK;
}

int ppde_chains_time_potts_kernel(ppde_chains* c, int reps, float* avg_us) {
    ARGCHK(c && c->initialised && avg_us && reps >= 1, "bad argument");
    ARGCHK(c->cfg.which & 1, "no Potts expert in this energy");
    HIPCHK(hipSetDevice(c->m->device));
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    hipEvent_t e0 = ev.a, e1 = ev.b;
    // writes the proposal slot, exactly as the launch inside an iteration does
    EvalTargets t = chain_targets(c, 1);
    int rc = launch_potts(c->m, cur_states(c), c->n, t, c->stream);   // warm
    if (rc) return rc;
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int i = 0; i < reps; ++i) {
        rc = launch_potts(c->m, cur_states(c), c->n, t, c->stream);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / reps;
    return PPDE_OK;
}

}  // extern "C"

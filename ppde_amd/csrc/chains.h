// The chains object of the C ABI (ppde_chains_*). Host code, included once, by ppde_api.hip behind the model and the expert launch
// layer. In this order: the modes' owner structs and the object; the rules the modes share; the modes, one header each (launch, fresh
// start, set / shape / read); the chain kernels' dispatcher, the iteration loop and its hipGraph capture; the object's entry points.
#pragma once

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

// forbidden patterns (ppde_chains_set_forbidden_patterns)
struct Forbidden {
    int M = 0, allow_native = 1;                 // patterns; the wild type's own matches are exempt
    std::vector<uint32_t> active, pattern;       // [L] bit m: pattern m is checked at that start; [32][8] element words (motif.h)
    DevBuf<uint32_t> active_dev, pattern_dev;
    DevBuf<uint8_t> veto;                        // [n] the pending proposal (or child) is not free
    DevBuf<long long> vetoes;                    // [n][M] iteration proposals vetoed, by lowest matching pattern
    bool on() const { return veto.p != nullptr; }
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
    Forbidden forbid;
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
    a.veto = c->forbid.veto;
    a.beta = c->anneal.on() ? c->anneal.beta.p : c->temper.beta.p; a.rung = c->temper.rung; a.slot = c->temper.slot; a.swap_attempts = c->temper.swap_attempts; a.swap_accepts = c->temper.swap_accepts;
    a.rung_hist = c->temper.rung_hist; a.n_rungs = c->temper.n_rungs; a.swap_every = c->temper.swap_every;
    return a;
}

static States cur_states(const ppde_chains* c) { return States{c->cur, c->curT, c->n_pad}; }
static States prop_states(const ppde_chains* c) { return States{c->prop, c->propT, c->n_pad}; }
static EvalTargets chain_targets(const ppde_chains* c, int slot) {
    EvalTargets t{c->grad, c->epart, c->gradC, c->fitC, slot, c->dbg};
    t.cmax = c->cnn_cmax; t.carg = c->cnn_carg; t.cgate = c->cnn_cgate; t.cnn_cap = c->n;
    t.gradT = c->gradT; t.tfE = c->tfE; t.tfw = c->tfw;
    return t;
}

// --------------------------------------------------------------------------------------------
// The rules the modes share. Each returns PPDE_OK or the refusal, composed as "function: shared sentence (the mode's reason)". An
// entry point makes its checks in the order it always has, and allocates, copies and launches nothing before the last of them.
#define CHK(x) do { const int rc_ = (x); if (rc_ != PPDE_OK) return rc_; } while (0)

static std::string at(const char* fn, const char* msg) { return std::string(fn) + ": " + msg; }

// a setter's first two checks: `what` ("the ladder", "pair counts") cannot change under the graphs captured at init, which hold `held`
static int set_before_init(const ppde_chains* c, const char* fn, const char* what, const char* held) {
    ARGCHK(c, "null argument");
    ARGCHK(!c->initialised, at(fn, what) + " must be set before ppde_chains_init (its graphs hold " + held + ")");
    return PPDE_OK;
}
static int needs_reversible(const ppde_chains* c, const char* fn, const char* mode, const char* why) {
    ARGCHK(c->reversible, at(fn, mode) + " needs reversible mode (ppde_chains_set_reversible): " + why);
    return PPDE_OK;
}
// the modes whose launches cover every chain of the object run on its one stream
static int one_stream(const ppde_chains* c, const char* fn, const char* why) {
    ARGCHK(c->streams.size() <= 1 && c->cfg.n_streams <= 1, at(fn, "n_streams > 1 is not supported (") + why + ")");
    return PPDE_OK;
}
// groups of `size` consecutive chains (ensembles of n_rungs, demes), counted from global chain 0: whole ones only in this shard
static int whole_groups(const ppde_chains* c, const char* fn, int size, const char* size_name, const char* groups, const char* a_group) {
    ARGCHK(c->n % size == 0, at(fn, "n_chains must be a multiple of ") + size_name + " (" + groups + ")");
    ARGCHK(c->cfg.chain_offset % (uint64_t)size == 0, at(fn, "chain_offset must be a multiple of ") + size_name + " (" + a_group +
                                                      " may not straddle two shards)");
    return PPDE_OK;
}
// two modes that exclude each other: the one that is set has to be cleared first, by `clear_call`
static int mode_not_set(bool is_set, const char* fn, const char* mode, const char* why, const char* clear_call) {
    ARGCHK(!is_set, at(fn, mode) + " is set (" + why + "); clear it first (" + clear_call + ")");
    return PPDE_OK;
}
// a reader's range of events against those that have happened (`shape_fn` reports them)
static int events_happened(const char* fn, int first_event, int n_events, int events_done, const char* shape_fn) {
    ARGCHK(first_event >= 0 && n_events >= 0 && first_event + n_events <= events_done,
           at(fn, "events beyond those that have happened (") + shape_fn + ")");
    return PPDE_OK;
}
// a setter called with NULL: the mode gives its buffers back
template <typename Mode>
static int clear_mode(ppde_chains* c, Mode& mode) {
    HIPCHK(hipSetDevice(c->device));
    mode = {};
    return PPDE_OK;
}

// One buffer of a mode's allocation list: `count` elements, zeroed or not, or filled from `count` host elements. alloc_all takes
// the list in order and stops at the first failure; the setter's local owner then releases what there is.
struct Alloc {
    hipError_t (*run)(const Alloc&);
    void* buf;
    size_t count;
    bool zero;
    const void* src;
    template <typename T>
    Alloc(DevBuf<T>& b, size_t count, bool zero = false, const void* src = nullptr)
        : run([](const Alloc& a) {
              DevBuf<T>& d = *(DevBuf<T>*)a.buf;
              const hipError_t e = a.zero ? d.alloc_zero(a.count) : d.alloc(a.count);
              return e != hipSuccess || !a.src ? e : hipMemcpy(d.p, a.src, a.count * sizeof(T), hipMemcpyHostToDevice);
          }),
          buf(&b), count(count), zero(zero), src(src) {}
    template <typename T>
    Alloc(DevBuf<T>& b, size_t count, const T* src) : Alloc(b, count, false, src) {}
};
static int alloc_all(const char* fn, std::initializer_list<Alloc> items) {
    for (const Alloc& a : items) {
        const hipError_t e = a.run(a);
        if (e != hipSuccess) return fail(PPDE_ERR_HIP, at(fn, "device allocation: ") + hipGetErrorString(e));
    }
    return PPDE_OK;
}

// rows [first, first + rows) of a device buffer [..][width] to the host; nothing for a NULL destination or an empty range
template <typename T>
static int copy_rows(void* dst, const T* src, size_t first, size_t rows, size_t width) {
    if (!dst || !rows || !width) return PPDE_OK;
    HIPCHK(hipMemcpy(dst, src + first * width, rows * width * sizeof(T), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

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

// --------------------------------------------------------------------------------------------
// The modes: everything the host knows about each (they need the object above; the loop below needs their launches and init their
// fresh starts).
#include "tempering_host.h"
#include "anneal_host.h"
#include "motif_host.h"
#include "recombine_host.h"
#include "record_host.h"
#include "pairs_host.h"
#include "archive_host.h"
#include "stats_host.h"

// --------------------------------------------------------------------------------------------
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
// Forbidden patterns: one veto launch on the proposal slot in front of every accept or fused launch, under both policies.
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
    bool after_event = false;                       // the previous iteration of this call ended with a recombination event
    for (int i = 0; i < count; ++i) {
        a.it_local = first_local + i;
        const bool event = c->recomb.on() && c->recomb.event(a.it_local);
        if (!c->cfg.reuse_grad) {   // energy and gradient at the current state (ppde.py:79)
            CHK(eval_experts(m, c->cfg.which, cur_states(c), c->n, chain_targets(c, 0), 1, s, b_off, n_sub));
        }
        if (!fuse || i == 0 || after_event) {
            CHK(launch_chain_kernel(c, KP_PROPOSE, a, n_sub, s));
        }
        // energy and gradient at the proposal (ppde.py:119)
        CHK(eval_experts(m, c->cfg.which, prop_states(c), c->n, chain_targets(c, 1), 1, s, b_off, n_sub));
        if (c->forbid.on()) CHK(launch_veto(c, b_off, n_sub, true, s));   // the proposal is not free: veto[b] for the accept phase
        CHK(launch_chain_kernel(c, (fuse && i + 1 < count && !event) ? KP_ACCEPT_PROPOSE : KP_ACCEPT, a, n_sub, s));
        after_event = event;
        // what follows runs on the object's one stream and covers every chain of it: the swap or the selection, then the observers,
        // which see the population those left
        if (c->temper.on()) CHK(launch_swap(c, a, s));
        if (c->anneal.on()) CHK(launch_select(c, it_base, a.it_local, s));
        if (event) CHK(launch_cross(c, it_base, a.it_local, s));
        if (c->recorder.on()) CHK(launch_record(c, it_base, a.it_local, s));
        if (c->pairs.on()) CHK(launch_pairs(c, it_base, a.it_local, s));      // (set only next to a recorder)
        if (c->archive.on()) CHK(launch_archive(c, it_base, a.it_local, s));
        if (c->stats.on()) CHK(launch_stats(c, it_base, a.it_local, U, mu_cap, s));
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
        CHK(enqueue_iterations(c, k, it_base, first_local, count, nullptr, nullptr, nullptr));
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

// The lengths of a chains object's graph segments, longest first: PPDE_GRAPH_LEN (one length) or {100, 20}. With recombination a
// segment holds its events at fixed places, so its length is a multiple of `every` and it is replayed from such positions only:
// PPDE_GRAPH_LEN if it is such a multiple, else the largest multiple of `every` up to 100 and `every` itself, or `every` alone
// when it lies in 101..1000.
static std::vector<int> segment_lengths(const ppde_chains* c) {
    static const int gl_read = env_int("PPDE_GRAPH_LEN", 0), gl_env = gl_read >= 1 && gl_read <= 1000 ? gl_read : 0;
    if (!c->recomb.on()) return gl_env ? std::vector<int>{gl_env} : std::vector<int>{100, 20};
    const int every = c->recomb.every;
    std::vector<int> lens;
    if (gl_env) { if (gl_env % every == 0) lens.push_back(gl_env); }
    else if (every <= 100) { lens.push_back(every * (100 / every)); if (lens[0] != every) lens.push_back(every); }
    else if (every <= 1000) lens.push_back(every);
    return lens;
}

// Graph segments of a chains object, each only if the histories can hold it. Captured and instantiated here, from
// ppde_chains_init, so that no ppde_chains_run pays for it.
static int capture_segments(ppde_chains* c) {
    if (!c->cfg.use_graph || c->cfg.rng_mode != 1 || !c->graphs.empty()) return PPDE_OK;
    if (c->cfg.which & 4) return PPDE_OK;           // ~900 launches per iteration, tens of milliseconds each way: nothing to gain from replay
    for (int len : segment_lengths(c))
        if (len <= c->T) CHK(capture_segment(c, len, false));
    return PPDE_OK;
}

// `reps` launches of `launch` on the object's stream between one event pair, after one warm launch: the mean in microseconds
template <typename F>
static int time_on_stream(ppde_chains* c, int reps, float* avg_us, F&& launch) {
    HIPCHK(hipSetDevice(c->m->device));
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    CHK(launch());   // warm
    HIPCHK(hipEventRecord(ev.a, c->stream));
    for (int i = 0; i < reps; ++i) CHK(launch());
    HIPCHK(hipEventRecord(ev.b, c->stream));
    HIPCHK(hipEventSynchronize(ev.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    *avg_us = ms * 1000.f / reps;
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
    CHK(set_before_init(c, __func__, "the library", "the pointer"));
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
    const char* fn = __func__;
    CHK(set_before_init(c, fn, "the mode", "the kernel choice"));
    ARGCHK(!(on && c->cfg.paper_results), "ppde_chains_set_reversible: paper_results restarts a rejected chain from its initial state, "
                                          "which is no Metropolis step; the two cannot be combined");
    // switching it off under a mode that needs it
    auto free_of = [&](bool is_set, const char* mode, const char* clear_call) -> int {
        ARGCHK(on || !is_set, at(fn, mode) + " is set and needs reversible mode (clear it with " + clear_call + " first)");
        return PPDE_OK;
    };
    CHK(free_of(c->temper.on(), "tempering", "ppde_chains_set_tempering(c, 0, NULL, 0)"));
    CHK(free_of(c->anneal.on(), "annealing", "ppde_chains_set_annealing(c, NULL)"));
    CHK(free_of(c->recomb.on(), "recombination", "ppde_chains_set_recombination(c, NULL)"));
    CHK(free_of(c->forbid.on(), "a pattern constraint", "ppde_chains_set_forbidden_patterns(c, NULL)"));
    c->reversible = on != 0;
    return PPDE_OK;
}

int ppde_chains_init(ppde_chains* c, const uint8_t* idx0_dev) {
    ARGCHK(c && idx0_dev, "null argument");
    ppde_model* m = c->m;
    HIPCHK(hipSetDevice(m->device));
    const Geom& g = m->g;
    hipStream_t s = c->stream;
    const int n = c->n;
    if (c->forbid.on()) CHK(forbidden_check_init(c, idx0_dev));    // every initial state must be free
    hipLaunchKernelGGL(k_pack_state, dim3((n * g.Ls + 255) / 256), dim3(256), 0, s, idx0_dev, c->cur, n, g.L, g.Ls, g.sh);
    HIPCHK(hipGetLastError());
    CHK(state_rows_to_t4(m, c->cur, c->curT, n, c->n_pad, s));
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
            CHK(eval_experts(m, c->cfg.which, fstates, nf, t, 1, s));
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
    CHK(eval_experts(m, c->cfg.which, cur_states(c), n, chain_targets(c, 0), 1, s));
    hipLaunchKernelGGL(k_init_chain, dim3((n + 3) / 4), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    if (c->cfg.reuse_grad) {   // the current state's combined gradient row travels with the chain from here on
        hipLaunchKernelGGL(k_combine_rows, dim3(n), dim3(256), 0, s, a, c->grad_cur);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    // a fresh start of every mode that is on (each in its header), then the graph segments
    if (c->temper.on()) CHK(tempering_fresh_start(c));
    if (c->anneal.on()) CHK(anneal_fresh_start(c));
    if (c->forbid.on()) CHK(forbidden_fresh_start(c));
    if (c->recorder.on()) CHK(recorder_fresh_start(c));
    if (c->pairs.on()) CHK(pairs_fresh_start(c));
    if (c->archive.on()) CHK(archive_fresh_start(c));
    if (c->stats.on()) CHK(stats_fresh_start(c));
    c->steps_done = 0;
    c->initialised = true;
    CHK(capture_segments(c));                       // (replayed by every later run; never captured inside one)
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
            CHK(enqueue_iterations(c, 0, nullptr, c->steps_done + i, 1, U_dev + (size_t)i * c->n, q_dev + qoff * c->n * g.N,
                                   u_dev + (size_t)i * c->n, max_u[i]));
            qoff += max_u[i];
        }
        c->steps_done += steps;
        return PPDE_OK;
    }
    // Replay: the longest captured segment that fits, as often as it fits, then what no segment covers as one eager block. With
    // recombination segments start at multiples of `every` only: eager iterations up to the next such position come first.
    const int every = c->recomb.on() && !c->graphs.empty() ? c->recomb.every : 1;
    int done = 0;
    while (done < steps) {
        const int pos = c->steps_done + done, left = steps - done;
        const ppde_chains::GraphSeg* seg = nullptr;
        if (pos % every == 0)
            for (const auto& gs : c->graphs) if (gs.len <= left) { seg = &gs; break; }       // longest first
        if (seg) {
            // every segment ends by adding its length to the device counter: it only needs setting after eager
            // iterations (which take their index from the launch arguments and leave the counter behind)
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
        CHK(enqueue_block(c, nullptr, pos, k));
        c->n_eager_steps += k;
        done += k;
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

int ppde_chains_peek(ppde_chains* c, uint8_t* idx, float* energy, float* fitness, uint8_t* accepted, int32_t* dist) {
    ARGCHK(c && c->initialised, "chains not initialised");
    CHK(ppde_chains_sync(c));
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
    CHK(ppde_chains_sync(c));
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

int ppde_chains_trace(ppde_chains* c, int32_t* flat, uint8_t* accepted, float* log_acc, int32_t* U) {
    ARGCHK(c && c->cfg.trace, "chains were created without trace");
    CHK(ppde_chains_sync(c));
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
    // current states into the proposal slot, exactly as the evaluation inside an iteration launches it
    return time_on_stream(c, reps, avg_us, [&] { return eval_experts(c->m, c->cfg.which, cur_states(c), c->n, chain_targets(c, 1), 1, c->stream); });
}

int ppde_chains_time_potts_kernel(ppde_chains* c, int reps, float* avg_us) {
    ARGCHK(c && c->initialised && avg_us && reps >= 1, "bad argument");
    ARGCHK(c->cfg.which & 1, "no Potts expert in this energy");
    // writes the proposal slot, exactly as the launch inside an iteration does
    return time_on_stream(c, reps, avg_us, [&] { return launch_potts(c->m, cur_states(c), c->n, chain_targets(c, 1), c->stream); });
}

}  // extern "C"

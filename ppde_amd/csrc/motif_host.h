// Forbidden patterns on the host: the plan (patterns and active words) a config gives, the veto launch, the free-state check of
// init, the fresh start, the setter and the readers, and the stateless scan. Included by chains.h, where the owner struct
// (Forbidden) stays with the others.
#pragma once

// what a ppde_motif_config says for a sequence of L residues: the [32][8] element words (0 behind each length) and active[L]
struct MotifPlan {
    int M = 0;
    std::vector<uint32_t> pattern, active;
    int native_m = -1, native_p = -1;            // allow_native = 0: the first (pattern, position) the wild type matches, or -1
};

// pattern m of `pattern` matches the plain row `x` [L] at start p
static bool motif_matches(const std::vector<uint32_t>& pattern, int m, int len, const uint8_t* x, int p) {
    for (int j = 0; j < len; ++j)
        if (!((pattern[(size_t)MOTIF_MAX_LEN * m + j] >> x[p + j]) & 1u)) return false;
    return true;
}

// the config's checks in the order of include/ppde_hip.h, then the plan; wt: the wild type's plain row [L]
static int motif_plan(const char* fn, const ppde_motif_config* cfg, int L, const uint8_t* wt, MotifPlan& out) {
    ARGCHK(cfg->n_patterns >= 1 && cfg->n_patterns <= MOTIF_MAX_PATTERNS, at(fn, "n_patterns must be in 1..32"));
    ARGCHK(cfg->length && cfg->element, at(fn, "null length or element array"));
    ARGCHK(L <= 0xffff, at(fn, "sequences longer than 65535 residues are not supported"));
    MotifPlan t;
    t.M = cfg->n_patterns;
    t.pattern.assign(MOTIF_WORDS, 0u);
    for (int m = 0; m < t.M; ++m) {
        const int len = cfg->length[m];
        ARGCHK(len >= 1 && len <= MOTIF_MAX_LEN, at(fn, "pattern ") + std::to_string(m) + ": length must be in 1..8");
        ARGCHK(len <= L, at(fn, "pattern ") + std::to_string(m) + ": length " + std::to_string(len) + " exceeds the sequence length " +
                             std::to_string(L));
        for (int j = 0; j < len; ++j) {
            const uint32_t e = cfg->element[(size_t)MOTIF_MAX_LEN * m + j];
            ARGCHK(e != 0u, at(fn, "pattern ") + std::to_string(m) + ", element " + std::to_string(j) + ": empty letter set");
            ARGCHK(!(e >> PPDE_A), at(fn, "pattern ") + std::to_string(m) + ", element " + std::to_string(j) + ": a bit >= 20 is set (20 letters)");
            t.pattern[(size_t)MOTIF_MAX_LEN * m + j] = e;
        }
    }
    t.active.assign((size_t)L, 0u);
    bool any = false;
    for (int m = 0; m < t.M; ++m) {
        const int len = cfg->length[m];
        for (int p = 0; p + len <= L; ++p) {
            const bool native = motif_matches(t.pattern, m, len, wt, p);
            if (native && cfg->allow_native) continue;
            if (native && t.native_m < 0) { t.native_m = m; t.native_p = p; }
            t.active[(size_t)p] |= 1u << m;
            any = true;
        }
    }
    ARGCHK(any, at(fn, "no active (pattern, position): the wild type matches every pattern at every start (allow_native)"));
    out = std::move(t);
    return PPDE_OK;
}

static MotifArgs motif_args(const uint8_t* rows, int stride, int sh, int L, int b_off, int n_sub, int M, const uint32_t* active,
                            const uint32_t* pattern) {
    MotifArgs r{};
    r.rows = rows; r.stride = stride; r.sh = sh; r.L = L; r.b_off = b_off; r.n_sub = n_sub; r.M = M;
    r.active = active; r.pattern = pattern;
    return r;
}

// the veto of the proposal slot's rows [b_off, b_off + n_sub) (motif.h); count: the iteration's launch bumps vetoes[b][m]
static int launch_veto(ppde_chains* c, int b_off, int n_sub, bool count, hipStream_t s) {
    const Geom& g = c->m->g;
    const Forbidden& fb = c->forbid;
    MotifArgs r = motif_args(c->prop, g.Ls, g.sh, g.L, b_off, n_sub, fb.M, fb.active_dev, fb.pattern_dev);
    r.veto = fb.veto;
    r.vetoes = count ? fb.vetoes.p : nullptr;
    launch_kernel(k_motif_veto, dim3((n_sub + MOTIF_NW - 1) / MOTIF_NW), dim3(MOTIF_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// first pattern and position of `n` plain rows [L] on the device -> the host
static int motif_scan_rows(const uint32_t* active_dev, const uint32_t* pattern_dev, int M, int L, const uint8_t* idx_dev, int n,
                           std::vector<int32_t>& fp, std::vector<int32_t>& fpos, hipStream_t s) {
    DevBuf<int> dp, dq;
    HIPCHK(dp.alloc((size_t)n));
    HIPCHK(dq.alloc((size_t)n));
    HIPCHK(hipMemsetAsync(dp, 0xff, (size_t)n * sizeof(int), s));   // -1: a row the launch does not reach reads as free
    MotifArgs r = motif_args(idx_dev, L, 0, L, 0, n, M, active_dev, pattern_dev);
    r.first_pattern = dp; r.first_pos = dq;
    launch_kernel(k_motif_scan, dim3((n + MOTIF_NW - 1) / MOTIF_NW), dim3(MOTIF_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    fp.resize((size_t)n); fpos.resize((size_t)n);
    HIPCHK(hipMemcpy(fp.data(), dp, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fpos.data(), dq, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return PPDE_OK;
}

// ppde_chains_init: every initial state must be free
static int forbidden_check_init(ppde_chains* c, const uint8_t* idx0_dev) {
    std::vector<int32_t> fp, fpos;
    CHK(motif_scan_rows(c->forbid.active_dev, c->forbid.pattern_dev, c->forbid.M, c->m->L, idx0_dev, c->n, fp, fpos, c->stream));
    for (int b = 0; b < c->n; ++b)
        if (fp[(size_t)b] >= 0)
            return fail(PPDE_ERR_INVALID, "ppde_chains_init: the initial state of chain " + std::to_string(b) + " is not free: forbidden pattern " +
                                          std::to_string(fp[(size_t)b]) + " matches at position " + std::to_string(fpos[(size_t)b]));
    return PPDE_OK;
}

static int forbidden_fresh_start(ppde_chains* c) {
    const Forbidden& fb = c->forbid;
    HIPCHK(hipMemsetAsync(fb.vetoes, 0, (size_t)c->n * fb.M * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(fb.veto, 0, (size_t)c->n, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_forbidden_patterns(ppde_chains* c, const ppde_motif_config* cfg) {
    const char* fn = __func__;
    CHK(set_before_init(c, fn, "the patterns", "the veto launches"));
    if (!cfg) return clear_mode(c, c->forbid);
    CHK(needs_reversible(c, fn, "a pattern constraint", "only there is the target exp(E) 1[free] / Z that the explicit rejection keeps"));
    MotifPlan plan;
    CHK(motif_plan(fn, cfg, c->m->L, c->m->h_wt.data(), plan));
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    Forbidden t;
    t.M = plan.M; t.allow_native = cfg->allow_native ? 1 : 0;
    CHK(alloc_all(fn, {{t.active_dev, plan.active.size(), plan.active.data()}, {t.pattern_dev, plan.pattern.size(), plan.pattern.data()},
                       {t.veto, (size_t)c->n, true}, {t.vetoes, (size_t)c->n * plan.M, true}}));
    t.active = std::move(plan.active);
    t.pattern = std::move(plan.pattern);
    c->forbid = std::move(t);
    g_err.clear();
    if (plan.native_m >= 0)                         // legal, and worth saying: no run can start from the wild type
        fail(PPDE_OK, at(fn, "note: the wild type matches pattern ") + std::to_string(plan.native_m) + " at position " +
                      std::to_string(plan.native_p) + " and allow_native is 0: it is not free, ppde_chains_init from it is refused");
    return PPDE_OK;
}

int ppde_chains_forbidden_shape(ppde_chains* c, int32_t* n_patterns, int32_t* allow_native, uint32_t* active) {
    ARGCHK(c, "null argument");
    ARGCHK(c->forbid.on(), "ppde_chains_forbidden_shape: no patterns were set (ppde_chains_set_forbidden_patterns)");
    if (n_patterns) *n_patterns = c->forbid.M;
    if (allow_native) *allow_native = c->forbid.allow_native;
    if (active) std::copy(c->forbid.active.begin(), c->forbid.active.end(), active);
    return PPDE_OK;
}

int ppde_chains_forbidden_read(ppde_chains* c, int64_t* vetoes) {
    ARGCHK(c && c->forbid.on(), "ppde_chains_forbidden_read: no patterns were set (ppde_chains_set_forbidden_patterns)");
    ARGCHK(c->initialised, "chains not initialised");
    CHK(ppde_chains_sync(c));
    return copy_rows(vetoes, c->forbid.vetoes.p, 0, (size_t)c->n, (size_t)c->forbid.M);
}

int ppde_motif_scan(ppde_model* m, const ppde_motif_config* cfg, const uint8_t* idx_dev, int n, int32_t* first_pattern_dev,
                    int32_t* first_pos_dev, void* stream) {
    const char* fn = __func__;
    ARGCHK(m && cfg && idx_dev && first_pattern_dev && first_pos_dev, "null argument");
    ARGCHK(n >= 1, at(fn, "need at least one row"));
    MotifPlan plan;
    CHK(motif_plan(fn, cfg, m->L, m->h_wt.data(), plan));
    HIPCHK(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf<uint32_t> active, pattern;
    CHK(alloc_all(fn, {{active, plan.active.size(), plan.active.data()}, {pattern, plan.pattern.size(), plan.pattern.data()}}));
    MotifArgs r = motif_args(idx_dev, m->L, 0, m->L, 0, n, plan.M, active, pattern);
    r.first_pattern = first_pattern_dev; r.first_pos = first_pos_dev;
    launch_kernel(k_motif_scan, dim3((n + MOTIF_NW - 1) / MOTIF_NW), dim3(MOTIF_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));                 // (the two buffers go with this call)
    return PPDE_OK;
}
}  // extern "C"

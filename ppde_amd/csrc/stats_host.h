// The move statistics on the host: their launch, their fresh start, the setter and the readers. Included by chains.h, where the owner
// struct (MoveStats) stays with the others: struct ppde_chains holds one of each by value, and all of this needs it complete.
#pragma once

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
    launch_kernel(k_stats, dim3(r.site_blocks + (c->n + STAT_NW - 1) / STAT_NW + 1), dim3(STAT_BLOCK), lds, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// a fresh start: zero counters, the initial population as the state before iteration 0
static int stats_fresh_start(ppde_chains* c) {
    hipStream_t s = c->stream;
    const int n = c->n;
    HIPCHK(hipMemsetAsync(c->stats.cnt, 0, c->stats.cells_total() * sizeof(long long), s));
    HIPCHK(hipMemcpyAsync(c->stats.prev, c->cur, (size_t)n * c->m->g.Ls, hipMemcpyDeviceToDevice, s));   // (buffer 0: iteration 0 reads it)
    hipLaunchKernelGGL(k_stats_init, dim3((n + 255) / 256), dim3(256), 0, s, c->rec, c->rec_stride, c->stats.dist, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_stats(ppde_chains* c, const ppde_stats_config* cfg) {
    CHK(set_before_init(c, __func__, "the statistics", "the pointers"));
    if (!cfg) return clear_mode(c, c->stats);
    ARGCHK(cfg->per_site == 0 || cfg->per_site == 1, "ppde_chains_set_stats: per_site must be 0 or 1");
    CHK(one_stream(c, __func__, "the counters have one owner per launch"));
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const Geom& g = c->m->g;
    MoveStats t;
    t.n = c->n; t.R = std::max(c->temper.n_rungs, 1); t.M = c->mu_max; t.L = g.L; t.per_site = cfg->per_site;
    CHK(alloc_all(__func__, {{t.cnt, t.cells_total(), true}, {t.prev, 2 * (size_t)t.n * g.Ls, true}, {t.dist, (size_t)t.n, true}}));
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
    CHK(ppde_chains_sync(c));
    int64_t* out[9] = {iters, accepts, moved, jump_sum, dist_sum, wt_returns, len_attempts, len_accepts, site_changes};
    for (int k = 0; k < 9; ++k) CHK(copy_rows(out[k], c->stats.counter(k), 0, 1, c->stats.cells(k)));
    return PPDE_OK;
}
}  // extern "C"

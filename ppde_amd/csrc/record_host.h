// The recorder on the host: its launch, its fresh start, the setter and the readers. Included by chains.h, where the owner struct
// (Recorder) stays with the others: struct ppde_chains holds one of each by value, and all of this needs it complete.
#pragma once

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
    launch_kernel(k_record, dim3(((g.Ls >> 2) + 3) / 4), dim3(REC_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// a fresh start counts from zero (the sample rows are written before they can be read)
static int recorder_fresh_start(ppde_chains* c) {
    HIPCHK(hipMemset(c->recorder.counts, 0, (size_t)c->m->g.L * PPDE_A * sizeof(unsigned long long)));
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_recorder(ppde_chains* c, const ppde_record_config* cfg) {
    const char* fn = __func__;
    CHK(set_before_init(c, fn, "the recorder", "the pointers"));
    ARGCHK(!c->pairs.on(), "ppde_chains_set_recorder: pair counts are set and follow this recorder's schedule; clear the pair counts first "
                           "(ppde_chains_set_pair_counts(c, NULL))");
    if (!cfg) return clear_mode(c, c->recorder);
    ARGCHK(cfg->every >= 1, "ppde_chains_set_recorder: every must be >= 1");
    ARGCHK(cfg->burn_in >= 0, "ppde_chains_set_recorder: negative burn_in");
    ARGCHK(cfg->rung >= -1, "ppde_chains_set_recorder: rung must be -1 (every chain) or a rung of the ladder");
    ARGCHK(cfg->keep_samples == 0 || cfg->keep_samples == 1, "ppde_chains_set_recorder: keep_samples must be 0 or 1");
    ARGCHK(cfg->rung < 0 || c->temper.on(), "ppde_chains_set_recorder: following a rung needs tempering (ppde_chains_set_tempering first)");
    ARGCHK(cfg->rung < c->temper.n_rungs || cfg->rung < 0, "ppde_chains_set_recorder: rung beyond the ladder");
    CHK(one_stream(c, fn, "the counters have one owner per launch"));
    const int rows_cap = c->T > cfg->burn_in ? (c->T - cfg->burn_in) / cfg->every : 0;
    ARGCHK(rows_cap >= 1, "ppde_chains_set_recorder: no iteration of max_steps would be recorded (burn_in + every > max_steps)");
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const Geom& g = c->m->g;
    const size_t slots = cfg->rung >= 0 ? (size_t)c->n / c->temper.n_rungs : (size_t)c->n, cells = (size_t)rows_cap * slots;
    Recorder t;
    t.cfg = *cfg; t.rows_cap = rows_cap; t.slots = (int)slots;
    CHK(alloc_all(fn, {{t.counts, (size_t)g.L * PPDE_A, true}}));
    if (cfg->keep_samples) CHK(alloc_all(fn, {{t.idx, cells * (size_t)g.Ls, true}, {t.e, cells}, {t.f, cells}, {t.chain, cells}}));
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
    CHK(ppde_chains_sync(c));
    const Geom& g = c->m->g;
    const Recorder& r = c->recorder;
    const size_t slots = r.slots, f = (size_t)first_row, k = (size_t)n_rows;
    if (idx && k * slots) CHK(read_state_rows(c, r.idx + f * slots * g.Ls, k, slots, idx));   // [rows][slots][Ls] -> [L]
    CHK(copy_rows(energy, r.e.p, f, k, slots));
    CHK(copy_rows(fitness, r.f.p, f, k, slots));
    CHK(copy_rows(chain, r.chain.p, f, k, slots));
    return copy_rows(site_counts, r.counts.p, 0, 1, (size_t)g.L * PPDE_A);
}
}  // extern "C"

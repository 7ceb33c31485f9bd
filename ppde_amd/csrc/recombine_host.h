// Recombination on the host: the event's launches, the setter and the readers; no fresh start (an event's rows are written before they
// can be read). Included by chains.h, where the owner struct (Recombination) stays with the others: struct ppde_chains holds one of
// each by value, and all of this needs it complete.
#pragma once

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
    launch_kernel(k_cross_propose, dim3(c->n / 2), dim3(CROSS_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    if (c->forbid.on()) CHK(launch_veto(c, 0, c->n, false, s));     // the children's bytes for outcome 4; not counted
    CHK(eval_experts(c->m, c->cfg.which, prop_states(c), c->n, chain_targets(c, 1), 1, s, 0, c->n));
    launch_kernel(k_cross_accept, dim3(c->n / 2), dim3(CROSS_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_recombination(ppde_chains* c, const ppde_recombine_config* cfg) {
    const char* fn = __func__;
    CHK(set_before_init(c, fn, "the mode", "the events"));
    if (!cfg) return clear_mode(c, c->recomb);
    CHK(needs_reversible(c, fn, "recombination", "only there do the chains have the law exp(E)/Z whose product the exchange keeps"));
    CHK(mode_not_set(c->temper.on(), fn, "tempering", "the decision takes no beta per chain", "ppde_chains_set_tempering(c, 0, NULL, 0)"));
    CHK(mode_not_set(c->anneal.on(), fn, "annealing", "the decision takes no beta per chain", "ppde_chains_set_annealing(c, NULL)"));
    ARGCHK(!c->cfg.paper_results, "ppde_chains_set_recombination: paper_results is not supported");
    ARGCHK(cfg->deme >= 2 && cfg->deme % 2 == 0, "ppde_chains_set_recombination: deme must be even and >= 2 (the chains of a deme are paired)");
    CHK(whole_groups(c, fn, cfg->deme, "deme", "demes of consecutive chains", "a deme"));
    ARGCHK(cfg->every >= 1, "ppde_chains_set_recombination: every must be >= 1");
    const int cap = c->T / cfg->every;
    ARGCHK(cap >= 1, "ppde_chains_set_recombination: no event would fit (events_cap = max_steps / every is 0)");
    CHK(one_stream(c, fn, "the exchange couples the chains of a deme"));
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
    CHK(alloc_all(fn, {{t.open_dev, t.open.size(), t.open.data()}, {t.partner, cells}, {t.lo, cells}, {t.hi, cells}, {t.differ, cells},
                       {t.child_dist, cells}, {t.outcome, cells}, {t.log_ratio, cells}, {t.pre, cells}, {t.child, cells}}));
    c->recomb = std::move(t);
    return PPDE_OK;
}

int ppde_chains_recombination_shape(ppde_chains* c, int32_t* deme, int32_t* n_open, int32_t* open_sites, int32_t* events_cap,
                                    int32_t* events_done) {
    ARGCHK(c, "null argument");
    ARGCHK(c->recomb.on(), "ppde_chains_recombination_shape: no recombination was set (ppde_chains_set_recombination)");
    ARGCHK(c->initialised, "chains not initialised");
    CHK(ppde_chains_sync(c));
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
    CHK(events_happened(__func__, first_event, n_events, c->recomb.events_done(c->steps_done), "ppde_chains_recombination_shape"));
    CHK(ppde_chains_sync(c));
    const Recombination& r = c->recomb;
    const size_t f = (size_t)first_event, k = (size_t)n_events, n = c->n;          // every buffer is [events_cap][n]
    CHK(copy_rows(partner, r.partner.p, f, k, n));
    CHK(copy_rows(lo, r.lo.p, f, k, n));
    CHK(copy_rows(hi, r.hi.p, f, k, n));
    CHK(copy_rows(differ, r.differ.p, f, k, n));
    CHK(copy_rows(child_dist, r.child_dist.p, f, k, n));
    CHK(copy_rows(outcome, r.outcome.p, f, k, n));
    CHK(copy_rows(log_ratio, r.log_ratio.p, f, k, n));
    CHK(copy_rows(pre_energy, r.pre.p, f, k, n));
    return copy_rows(child_energy, r.child.p, f, k, n);
}
}  // extern "C"

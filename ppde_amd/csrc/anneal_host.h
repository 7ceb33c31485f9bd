// Population annealing on the host, fixed and adaptive: the selection's launches, the fresh start, the two setters (one body) and the
// readers. Included by chains.h, where the owner struct (Annealing) stays with the others: struct ppde_chains holds one of each by
// value, and all of this needs it complete.
#pragma once

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
        launch_kernel(k_select_plan_adaptive, dim3(c->n / c->anneal.D), dim3(ANNEAL_BLOCK), 0, s, nullptr, r, x);
    } else {
        launch_kernel(k_select_plan, dim3(c->n / c->anneal.D), dim3(ANNEAL_BLOCK), 0, s, nullptr, r);
    }
    HIPCHK(hipGetLastError());
    launch_kernel(k_select_copy, dim3(c->n), dim3(ANNEAL_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// a fresh start: every chain at beta[0]
static int anneal_fresh_start(ppde_chains* c) {
    const std::vector<float> hb((size_t)c->n, c->anneal.sched[0]);
    HIPCHK(hipMemcpy(c->anneal.beta, hb.data(), (size_t)c->n * sizeof(float), hipMemcpyHostToDevice));
    return PPDE_OK;
}

// What a setter brings: the fields both forms have, the schedule as the device gets it (fixed: beta[0..S]; adaptive: beta_start,
// beta_end), and the adaptive form's two numbers.
struct AnnealForm {
    int deme, every, stages;
    const char* stages_name;                     // n_stages / max_stages
    const float* sched;
    size_t n_sched;
    bool adaptive;
    float rho, min_step;
};

// The one body of ppde_chains_set_annealing and ppde_chains_set_annealing_adaptive. `what`: what "must be set before
// ppde_chains_init" in the form's words; `f` NULL clears; `own_checks` are the form's checks of its schedule, made where both
// forms have always made them: after the event count, before the stream count.
template <typename Own>
static int set_annealing(ppde_chains* c, const char* fn, const char* what, const AnnealForm* f, Own&& own_checks) {
    CHK(set_before_init(c, fn, what, "the kernel choice"));
    CHK(mode_not_set(c->recomb.on(), fn, "recombination", "its decision takes no beta per chain", "ppde_chains_set_recombination(c, NULL)"));
    if (!f) return clear_mode(c, c->anneal);
    CHK(needs_reversible(c, fn, "annealing", "only there is the law at beta, exp(beta E)/Z, defined"));
    CHK(mode_not_set(c->temper.on(), fn, "tempering", "a schedule and a ladder cannot be combined", "ppde_chains_set_tempering(c, 0, NULL, 0)"));
    ARGCHK(f->deme >= 2 && f->deme <= ANNEAL_DMAX, at(fn, "deme must be in 2..1024"));
    CHK(whole_groups(c, fn, f->deme, "deme", "demes of consecutive chains", "a deme"));
    ARGCHK(f->every >= 1, at(fn, "every must be >= 1"));
    ARGCHK(f->stages >= 1 && f->stages <= 4096, at(fn, f->stages_name) + " must be in 1..4096");
    ARGCHK(f->sched, at(fn, "no schedule (beta is NULL)"));
    const int cap = std::min(f->stages, c->T / f->every);
    ARGCHK(cap >= 1, at(fn, "no event would fit (events_cap = min(") + f->stages_name + ", max_steps / every) is 0)");
    CHK(own_checks());
    CHK(one_stream(c, fn, "the selection couples the chains of a deme"));
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, demes = n / f->deme, events = (size_t)cap;
    Annealing t;
    t.D = f->deme; t.every = f->every; t.S = f->stages; t.cap = cap;
    t.adaptive = f->adaptive; t.rho = f->rho; t.min_step = f->min_step;
    t.sched.assign(f->sched, f->sched + f->n_sched);
    CHK(alloc_all(fn, {{t.sched_dev, f->n_sched, f->sched}, {t.beta, n}, {t.pre, events * n}, {t.parent, events * n},
                       {t.lmw, events * demes}, {t.ess, events * demes}}));
    if (f->adaptive) CHK(alloc_all(fn, {{t.beta_pair, 2 * events * demes}}));
    c->anneal = std::move(t);
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_annealing(ppde_chains* c, const ppde_anneal_config* cfg) {
    const char* fn = __func__;
    AnnealForm f{};
    if (cfg) f = {cfg->deme, cfg->every, cfg->n_stages, "n_stages", cfg->beta, (size_t)cfg->n_stages + 1, false, 0.f, 0.f};
    return set_annealing(c, fn, "the schedule", cfg ? &f : nullptr, [&]() -> int {
        for (int s = 0; s <= cfg->n_stages; ++s) {
            const float b = cfg->beta[s];
            if (!(b > 0.f) || !(b < INFINITY))
                return fail(PPDE_ERR_INVALID, "ppde_chains_set_annealing: beta[" + std::to_string(s) + "] must be finite and positive");
            if (s > 0 && b < cfg->beta[s - 1])
                return fail(PPDE_ERR_INVALID, "ppde_chains_set_annealing: the schedule must not decrease (beta[" + std::to_string(s) +
                                              "] < beta[" + std::to_string(s - 1) + "])");
        }
        return PPDE_OK;
    });
}

int ppde_chains_set_annealing_adaptive(ppde_chains* c, const ppde_anneal_adaptive_config* cfg) {
    const char* fn = __func__;
    AnnealForm f{};
    float pair[2] = {0.f, 0.f};
    if (cfg) {
        pair[0] = cfg->beta_start; pair[1] = cfg->beta_end;
        f = {cfg->deme, cfg->every, cfg->max_stages, "max_stages", pair, 2, true, cfg->ess_target, cfg->min_step};
    }
    return set_annealing(c, fn, "the mode", cfg ? &f : nullptr, [&]() -> int {
        ARGCHK(cfg->beta_start > 0.f && cfg->beta_start < INFINITY, "ppde_chains_set_annealing_adaptive: beta_start must be finite and positive");
        ARGCHK(cfg->beta_end > 0.f && cfg->beta_end < INFINITY, "ppde_chains_set_annealing_adaptive: beta_end must be finite and positive");
        ARGCHK(cfg->beta_start < cfg->beta_end, "ppde_chains_set_annealing_adaptive: beta_start must be below beta_end");
        ARGCHK(cfg->ess_target > 0.f && cfg->ess_target < 1.f, "ppde_chains_set_annealing_adaptive: ess_target must be inside (0, 1)");
        ARGCHK(cfg->min_step < INFINITY && cfg->min_step >= cfg->beta_end * 0x1p-20f,
               "ppde_chains_set_annealing_adaptive: min_step must be finite and >= beta_end * 2^-20 (a step that changes beta in fp32)");
        return PPDE_OK;
    });
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
    CHK(events_happened(__func__, first_event, n_events, c->anneal.events_done(c->steps_done), "ppde_chains_annealing_shape"));
    CHK(ppde_chains_sync(c));
    const Annealing& an = c->anneal;
    const size_t n = c->n, demes = n / an.D, f = (size_t)first_event, k = (size_t)n_events;
    CHK(copy_rows(parent, an.parent.p, f, k, n));
    CHK(copy_rows(pre_energy, an.pre.p, f, k, n));
    CHK(copy_rows(log_mean_w, an.lmw.p, f, k, demes));
    CHK(copy_rows(ess, an.ess.p, f, k, demes));
    return copy_rows(beta_now, an.beta.p, 0, 1, n);
}

int ppde_chains_annealing_read_betas(ppde_chains* c, int first_event, int n_events, float* beta_before, float* beta_after) {
    ARGCHK(c && c->anneal.on(), "ppde_chains_annealing_read_betas: no annealing was set (ppde_chains_set_annealing)");
    ARGCHK(c->initialised, "chains not initialised");
    CHK(events_happened(__func__, first_event, n_events, c->anneal.events_done(c->steps_done), "ppde_chains_annealing_shape"));
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
    CHK(ppde_chains_sync(c));
    CHK(copy_rows(beta_before, an.beta_pair.p, f, k, demes));                          // [2][events_cap][n/D]: before, then after
    return copy_rows(beta_after, an.beta_pair.p, (size_t)an.cap + f, k, demes);
}
}  // extern "C"

// Parallel tempering on the host: the swap's launch, the fresh start, the setter and the two readers. Included by chains.h, where the
// owner struct (Tempering) stays with the others: struct ppde_chains holds one of each by value, and all of this needs it complete.
#pragma once

// the swap behind the accept phase of the iteration in `a` (pas.h k_swap): every chain of the object, on its one stream
static int launch_swap(ppde_chains* c, const PasArgs& a, hipStream_t s) {
    launch_kernel(k_swap, dim3((c->n + 255) / 256), dim3(256), 0, s, nullptr, a);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// rungs, temperatures, slots and counters of a fresh start: chain g = chain_offset + b starts on rung g % R (chain_offset % R == 0)
static int tempering_fresh_start(ppde_chains* c) {
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

extern "C" {
int ppde_chains_set_tempering(ppde_chains* c, int n_rungs, const float* beta_host, int swap_every) {
    const char* fn = __func__;
    CHK(set_before_init(c, fn, "the ladder", "the kernel choice"));
    ARGCHK(!(c->recorder.on() && c->recorder.cfg.rung >= 0), "ppde_chains_set_tempering: a recorder that follows a rung is set; clear it first "
                                                             "(ppde_chains_set_recorder(c, NULL))");
    ARGCHK(!c->stats.on(), "ppde_chains_set_tempering: move statistics are set and were shaped by the ladder there was; clear them first "
                           "(ppde_chains_set_stats(c, NULL))");
    CHK(mode_not_set(c->anneal.on(), fn, "annealing", "a schedule and a ladder cannot be combined", "ppde_chains_set_annealing(c, NULL)"));
    CHK(mode_not_set(c->recomb.on(), fn, "recombination", "its decision takes no beta per chain", "ppde_chains_set_recombination(c, NULL)"));
    HIPCHK(hipSetDevice(c->device));
    if (n_rungs == 0 || !beta_host) {               // clear
        c->temper = {};
        return PPDE_OK;
    }
    const int R = n_rungs;
    CHK(needs_reversible(c, fn, "tempering", "only there is the law at beta, exp(beta E)/Z, defined"));
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
    CHK(whole_groups(c, fn, R, "n_rungs", "ensembles of n_rungs consecutive chains", "an ensemble"));
    CHK(one_stream(c, fn, "the swap couples the chains of an ensemble"));
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, pairs = (n / R) * (size_t)(R - 1);
    Tempering t;
    t.n_rungs = R; t.swap_every = swap_every;
    t.ladder.assign(beta_host, beta_host + R);
    CHK(alloc_all(fn, {{t.beta, n}, {t.rung, n}, {t.slot, n}, {t.swap_attempts, pairs}, {t.swap_accepts, pairs},
                       {t.rung_hist, ((size_t)c->T + 1) * n}}));
    c->temper = std::move(t);
    return PPDE_OK;
}

int ppde_chains_tempering_state(ppde_chains* c, int32_t* rung, float* beta, int64_t* swap_attempts, int64_t* swap_accepts) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(c->temper.on(), "ppde_chains_tempering_state: no tempering was set (ppde_chains_set_tempering)");
    CHK(ppde_chains_sync(c));
    const size_t n = c->n, pairs = (n / c->temper.n_rungs) * (size_t)(c->temper.n_rungs - 1);
    CHK(copy_rows(rung, c->temper.rung.p, 0, 1, n));
    CHK(copy_rows(beta, c->temper.beta.p, 0, 1, n));
    CHK(copy_rows(swap_attempts, c->temper.swap_attempts.p, 0, 1, pairs));
    return copy_rows(swap_accepts, c->temper.swap_accepts.p, 0, 1, pairs);
}

int ppde_chains_tempering_history(ppde_chains* c, uint8_t* rung_history) {
    ARGCHK(c && c->initialised && rung_history, "chains not initialised, or null argument");
    ARGCHK(c->temper.on(), "ppde_chains_tempering_history: no tempering was set (ppde_chains_set_tempering)");
    CHK(ppde_chains_sync(c));
    return copy_rows(rung_history, c->temper.rung_hist.p, 0, (size_t)c->steps_done + 1, (size_t)c->n);
}
}  // extern "C"

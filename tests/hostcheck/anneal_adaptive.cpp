// TEST INFRASTRUCTURE. Adaptive population annealing's host side (ppde_chains_set_annealing_adaptive,
// ppde_chains_annealing_read_betas, and ppde_chains_annealing_shape / _read serving it; include/ppde_hip.h) against the mock runtime
// of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_reversible -> set_annealing_adaptive (every refusal,
// then a valid configuration) -> shape -> init -> run -> both reads -> clear -> replacement by the fixed form and back, eager and
// from captured graphs, and -- with `driver sweep` -- the same walk once per fallible runtime call with that call failing, so every
// clean-up path runs. Kernels do not run here: numbers mean nothing, memory errors and leaks are the point. It follows anneal.cpp.
#include "walk.h"

namespace {
ppde_anneal_adaptive_config xcfg(int deme, int every, int stages, float b0, float b1, float rho, float min_step) {
    ppde_anneal_adaptive_config a{};
    a.deme = deme; a.every = every; a.max_stages = stages; a.beta_start = b0; a.beta_end = b1; a.ess_target = rho; a.min_step = min_step;
    return a;
}
ppde_anneal_config acfg(int deme, int every, int stages, const float* beta) { ppde_anneal_config a{}; a.deme = deme; a.every = every; a.n_stages = stages; a.beta = beta; return a; }

int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cs = nullptr, *cn = nullptr;
    const int n = 8, T = 30, N = L * 20;
    const float sched[4] = {0.125f, 0.25f, 0.5f, 1.0f};
    const float ladder[2] = {1.0f, 0.5f};
    const float step = 0x1p-12f;
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    TRY(ppde_model_create(&m, 0, L, wt.data()));
    {
        auto J = rnd((size_t)Lp * Lp * 400, 0.05f), h = rnd((size_t)Lp * 20, 0.5f);
        TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));
        const int C = L, K = 5, F = 2 * L;
        auto cw = many(3, (size_t)C * 20 * K), cb = many(3, C), lw = many(3, (size_t)F * C), lb = many(3, F), dw = many(3, F), db = many(3, 1);
        TRY(ppde_model_set_cnn(m, 3, C, K, F, cw.p.data(), cb.p.data(), lw.p.data(), lb.p.data(), dw.p.data(), db.p.data()));
        TRY(ppde_model_set_lamda(m, 5.0f));
    }
    {
        // caller-supplied noise, eager: an event every 2nd iteration, at most 3
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        ppde_anneal_adaptive_config good = xcfg(4, 2, 3, 0.125f, 1.0f, 0.5f, step);
        ppde_anneal_config fixed = acfg(4, 2, 3, sched);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &good), "reversible");     // reversible mode not on
            EXPECT_INVALID(ppde_chains_annealing_shape(c0, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_set_reversible(c0, 1));
        if (refusals) {
            ppde_anneal_adaptive_config a;
            EXPECT_INVALID(ppde_chains_set_annealing_adaptive(nullptr, &good));
            a = good; a.deme = 1; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "2..1024");
            a = good; a.deme = 1025; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "2..1024");
            a = good; a.deme = 3; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "multiple");   // 8 chains are no multiple of 3
            a = good; a.every = 0; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "every");
            a = good; a.every = T + 1; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "no event");   // events_cap == 0
            a = good; a.max_stages = 0; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "max_stages");
            a = good; a.max_stages = 4097; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "max_stages");
            a = good; a.beta_start = 0.f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "beta_start");
            a = good; a.beta_start = -1.f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "beta_start");
            a = good; a.beta_start = NAN; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "beta_start");
            a = good; a.beta_end = INFINITY; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "beta_end");
            a = good; a.beta_end = NAN; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "beta_end");
            a = good; a.beta_start = 1.0f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "below");
            a = good; a.beta_start = 2.0f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "below");
            a = good; a.ess_target = 0.f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "ess_target");
            a = good; a.ess_target = 1.f; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "ess_target");
            a = good; a.ess_target = NAN; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "ess_target");
            a = good; a.min_step = NAN; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "min_step");
            a = good; a.min_step = INFINITY; EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "min_step");
            a = good; a.min_step = std::nextafter(0x1p-20f, 0.f); EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &a), "min_step");
        }
        {
            ppde_anneal_adaptive_config a = xcfg(2, T, 4096, 0.5f, 1.0f, std::nextafter(1.0f, 0.f), 0x1p-20f);   // the accepted edges
            TRY(ppde_chains_set_annealing_adaptive(c0, &a));
        }
        TRY(ppde_chains_set_annealing_adaptive(c0, nullptr));                         // cleared
        TRY(ppde_chains_set_reversible(c0, 0));                                       // (nothing set: switching the mode off is fine)
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_tempering(c0, 2, ladder, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &good), "tempering");   // a ladder is set
        TRY(ppde_chains_set_tempering(c0, 0, nullptr, 0));
        // replacement: adaptive -> fixed -> adaptive, then cleared through the OTHER setter and set again
        TRY(ppde_chains_set_annealing_adaptive(c0, &good));
        TRY(ppde_chains_set_annealing(c0, &fixed));
        TRY(ppde_chains_set_annealing_adaptive(c0, &good));
        TRY(ppde_chains_set_annealing(c0, nullptr));
        if (refusals) EXPECT_INVALID(ppde_chains_annealing_shape(c0, nullptr, nullptr, nullptr));
        TRY(ppde_chains_set_annealing(c0, &fixed));
        TRY(ppde_chains_set_annealing_adaptive(c0, nullptr));
        if (refusals) EXPECT_INVALID(ppde_chains_annealing_shape(c0, nullptr, nullptr, nullptr));
        TRY(ppde_chains_set_annealing_adaptive(c0, &good));
        if (refusals) {
            ppde_recombine_config rc{}; rc.deme = 4; rc.every = 2;
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 0));                        // annealing needs the mode
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, ladder, 1));              // ... and excludes a ladder
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 0, nullptr, 0));
            EXPECT_INVALID(ppde_chains_set_recombination(c0, &rc), "annealing");      // ... and recombination
            std::vector<float> bb(2);
            EXPECT_INVALID(ppde_chains_annealing_read_betas(c0, 0, 0, bb.data(), bb.data()));   // before init
        }
        int32_t deme = 0, cap = 0, done_ev = -1;
        TRY(ppde_chains_annealing_shape(c0, &deme, &cap, &done_ev));
        if (deme != 4 || cap != 3 || done_ev != 0) { fprintf(stderr, "annealing shape before init %d %d %d\n", deme, cap, done_ev); status = 94; goto done; }
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, &good));            // after init: the graphs hold the kernel choice
            EXPECT_INVALID(ppde_chains_set_annealing_adaptive(c0, nullptr));
        }
        const int steps = 5;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        TRY(ppde_chains_annealing_shape(c0, &deme, &cap, &done_ev));
        if (deme != 4 || cap != 3 || done_ev != 2) { fprintf(stderr, "annealing shape %d %d %d\n", deme, cap, done_ev); status = 94; goto done; }
        std::vector<int32_t> par((size_t)done_ev * n);
        std::vector<float> pre((size_t)done_ev * n), beta(n), before((size_t)done_ev * (n / 4)), after((size_t)done_ev * (n / 4));
        std::vector<double> lmw((size_t)done_ev * (n / 4)), ess((size_t)done_ev * (n / 4));
        TRY(ppde_chains_annealing_read(c0, 0, done_ev, par.data(), pre.data(), lmw.data(), ess.data(), beta.data()));
        TRY(ppde_chains_annealing_read_betas(c0, 0, done_ev, before.data(), after.data()));
        TRY(ppde_chains_annealing_read_betas(c0, 1, 1, before.data(), nullptr));
        TRY(ppde_chains_annealing_read_betas(c0, 1, 1, nullptr, after.data()));
        TRY(ppde_chains_annealing_read_betas(c0, 2, 0, nullptr, nullptr));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_annealing_read_betas(c0, 0, done_ev + 1, before.data(), after.data()), "beyond");
            EXPECT_INVALID(ppde_chains_annealing_read_betas(c0, -1, 1, before.data(), after.data()), "beyond");
            EXPECT_INVALID(ppde_chains_annealing_read_betas(c0, 2, 1, before.data(), after.data()), "beyond");
            EXPECT_INVALID(ppde_chains_annealing_read_betas(nullptr, 0, 0, nullptr, nullptr));
        }
        for (int b = 0; b < n; ++b)
            if (beta[b] != 0.125f) { fprintf(stderr, "start temperatures\n"); status = 93; goto done; }   // (kernels do not run here)
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold the *_temp kernels, the adaptive plan and the copy), replayed, then an eager
        // remainder; the second object has all chains in one deme and runs past max_stages
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = reuse ? 2 : -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 104;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        TRY(ppde_chains_set_reversible(c, 1));
        ppde_anneal_adaptive_config a = xcfg(reuse ? n : 2, reuse ? 4 : 7, 3, 0.25f, 1.0f, 0.75f, step);
        TRY(ppde_chains_set_annealing_adaptive(c, &a));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t deme = 0, ecap = 0, edone = 0;
        TRY(ppde_chains_annealing_shape(c, &deme, &ecap, &edone));
        if (ecap != 3 || edone != 3) { fprintf(stderr, "events %d of %d\n", edone, ecap); status = 92; goto done; }
        std::vector<float> before((size_t)edone * (n / deme)), after((size_t)edone * (n / deme));
        TRY(ppde_chains_annealing_read_betas(c, 0, edone, before.data(), after.data()));
        TRY(ppde_chains_init(c, idx.data()));                                     // a second start
        TRY(ppde_chains_annealing_shape(c, nullptr, nullptr, &edone));
        if (edone != 0) { fprintf(stderr, "events after a second init: %d\n", edone); status = 91; goto done; }
    }
    {
        // the fixed form answers read_betas from its schedule; what the shape of the object refuses: a shard that cuts a deme, two streams
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 6; cfg.n_streams = 1;
        TRY(ppde_chains_create(&cs, m, &cfg));
        TRY(ppde_chains_set_reversible(cs, 1));
        ppde_anneal_adaptive_config a4 = xcfg(4, 1, 3, 0.25f, 1.0f, 0.5f, step), a2 = xcfg(2, 1, 3, 0.25f, 1.0f, 0.5f, step);
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing_adaptive(cs, &a4), "chain_offset");   // 6 is no multiple of 4
        TRY(ppde_chains_set_annealing_adaptive(cs, &a2));                                             // ... but of 2
        ppde_anneal_config f2 = acfg(2, 1, 3, sched);
        TRY(ppde_chains_set_annealing(cs, &f2));
        TRY(ppde_chains_init(cs, idx.data()));
        TRY(ppde_chains_run(cs, 2, nullptr, nullptr, nullptr, nullptr));
        std::vector<float> before(2 * (n / 2)), after(2 * (n / 2));
        TRY(ppde_chains_annealing_read_betas(cs, 0, 2, before.data(), after.data()));
        for (int d = 0; d < n / 2; ++d)
            if (before[d] != sched[0] || after[d] != sched[1] || before[n / 2 + d] != sched[1] || after[n / 2 + d] != sched[2]) {
                fprintf(stderr, "the fixed schedule's beta pairs\n"); status = 90; goto done;
            }
        if (refusals) EXPECT_INVALID(ppde_chains_annealing_read_betas(cs, 0, 3, before.data(), after.data()), "beyond");
        cfg.chain_offset = 0; cfg.n_streams = 2;
        TRY(ppde_chains_create(&cn, m, &cfg));
        TRY(ppde_chains_set_reversible(cn, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing_adaptive(cn, &a4), "n_streams");       // two streams
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) EXPECT_INVALID(ppde_chains_annealing_read_betas(cn, 0, 0, nullptr, nullptr));
        TRY(ppde_chains_run(cn, 5, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(cn));
    }
done:
    if (cs) ppde_chains_destroy(cs);
    if (cn) ppde_chains_destroy(cn);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck anneal_adaptive ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

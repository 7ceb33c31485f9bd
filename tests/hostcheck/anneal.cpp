// TEST INFRASTRUCTURE. Population annealing's host side (ppde_chains_set_annealing, ppde_chains_annealing_shape / _read,
// include/ppde_hip.h) against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_library ->
// set_reversible -> set_annealing (every refusal, then a valid schedule) -> init -> run -> annealing_shape / read -> collect ->
// destroy on both RNG modes and both gradient policies (eager and from captured graphs), and -- with `driver sweep` -- the same walk
// once per fallible runtime call with that call failing, so every clean-up path runs. Kernels do not run here: numbers mean
// nothing, memory errors and leaks are the point.
#include "walk.h"

namespace {
ppde_anneal_config acfg(int deme, int every, int stages, const float* beta) { ppde_anneal_config a{}; a.deme = deme; a.every = every; a.n_stages = stages; a.beta = beta; return a; }

// the walk; returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer)
int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cs = nullptr, *cn = nullptr;
    const int n = 8, T = 30, N = L * 20;
    const float sched[4] = {0.125f, 0.25f, 0.5f, 1.0f};
    const float ladder[2] = {1.0f, 0.5f};
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    std::vector<uint32_t> lib(L, 0u);
    for (int l = win; l < win + Lp; ++l)
        if (l % 3) lib[l] = (1u << wt[l]) | (1u << ((wt[l] + 3) % 20)) | (1u << ((wt[l] + 7) % 20)) | (1u << ((wt[l] + 11) % 20)) | (1u << ((wt[l] + 16) % 20));
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
        // caller-supplied noise (flat race), trace on, a mutation cap: the *_temp kernels in their replay form, a stage every 2nd iteration
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        TRY(ppde_chains_set_library(c0, lib.data()));
        ppde_anneal_config good = acfg(4, 2, 3, sched);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_annealing(c0, &good));                    // reversible mode not on
            if (!strstr(ppde_last_error(), "reversible")) { fprintf(stderr, "the refusal does not name reversible mode: %s\n", ppde_last_error()); status = 95; goto done; }
            EXPECT_INVALID(ppde_chains_annealing_shape(c0, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_set_reversible(c0, 1));
        if (refusals) {
            std::vector<float> big(4098, 1.0f);
            const float down[2] = {1.0f, 0.5f}, zero[2] = {0.0f, 1.0f}, neg[2] = {-1.0f, 1.0f}, nan2[2] = {0.5f, NAN}, inf2[2] = {0.5f, INFINITY};
            ppde_anneal_config a;
            EXPECT_INVALID(ppde_chains_set_annealing(nullptr, &good));
            a = acfg(1, 2, 3, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(1025, 2, 3, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(3, 2, 3, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));      // 8 chains are no multiple of 3
            a = acfg(4, 0, 3, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 0, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 4097, big.data()); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, T + 1, 3, sched); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a)); // events_cap == 0
            a = acfg(4, 2, 3, nullptr); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 1, down); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 1, zero); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 1, neg); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 1, nan2); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
            a = acfg(4, 2, 1, inf2); EXPECT_INVALID(ppde_chains_set_annealing(c0, &a));
        }
        {
            std::vector<float> ones(4097, 1.0f);
            ppde_anneal_config a = acfg(2, T, 4096, ones.data());                 // the accepted edges, replaced below
            TRY(ppde_chains_set_annealing(c0, &a));
        }
        TRY(ppde_chains_set_annealing(c0, nullptr));                              // cleared, then the schedule the run uses
        TRY(ppde_chains_set_reversible(c0, 0));                                   // (no annealing set: switching the mode off is fine)
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_tempering(c0, 2, ladder, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing(c0, &good));       // a ladder is set
        TRY(ppde_chains_set_tempering(c0, 0, nullptr, 0));
        TRY(ppde_chains_set_annealing(c0, &good));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 0));                    // annealing needs the mode
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, ladder, 1));          // ... and excludes a ladder
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 0, nullptr, 0));
            std::vector<int32_t> par(n);
            EXPECT_INVALID(ppde_chains_annealing_read(c0, 0, 0, par.data(), nullptr, nullptr, nullptr, nullptr));   // before init
        }
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_annealing(c0, &good));                 // after init: the graphs hold the kernel choice
            EXPECT_INVALID(ppde_chains_set_annealing(c0, nullptr));
        }
        const int steps = 5;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        int32_t deme = 0, cap = 0, done_ev = 0;
        TRY(ppde_chains_annealing_shape(c0, &deme, &cap, &done_ev));
        TRY(ppde_chains_annealing_shape(c0, nullptr, nullptr, nullptr));
        if (deme != 4 || cap != 3 || done_ev != 2) { fprintf(stderr, "annealing shape %d %d %d\n", deme, cap, done_ev); status = 94; goto done; }
        std::vector<int32_t> par((size_t)done_ev * n), bs(n);
        std::vector<float> pre((size_t)done_ev * n), beta(n), be(n), bf(n), eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        std::vector<double> lmw((size_t)done_ev * (n / 4)), ess((size_t)done_ev * (n / 4));
        std::vector<uint8_t> bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        TRY(ppde_chains_annealing_read(c0, 0, done_ev, par.data(), pre.data(), lmw.data(), ess.data(), beta.data()));
        TRY(ppde_chains_annealing_read(c0, 1, 1, par.data(), pre.data(), lmw.data(), ess.data(), nullptr));
        TRY(ppde_chains_annealing_read(c0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_annealing_read(c0, 0, done_ev + 1, par.data(), nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_annealing_read(c0, -1, 1, par.data(), nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_annealing_read(c0, 2, 1, par.data(), nullptr, nullptr, nullptr, nullptr));
        }
        for (int b = 0; b < n; ++b)
            if (beta[b] != sched[0]) { fprintf(stderr, "start temperatures\n"); status = 93; goto done; }   // (kernels do not run here)
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        if (ppde_chains_steps_done(c0) != steps) { fprintf(stderr, "steps_done\n"); status = 97; goto done; }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold the *_temp kernels and the two selection kernels), replayed, then an eager
        // remainder; the second object runs WITHOUT a library, all chains in one deme, past the end of its schedule
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = reuse ? 2 : -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 104;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        if (!reuse) TRY(ppde_chains_set_library(c, lib.data()));
        TRY(ppde_chains_set_reversible(c, 1));
        ppde_anneal_config a = acfg(reuse ? n : 2, reuse ? 4 : 7, 3, sched);
        TRY(ppde_chains_set_annealing(c, &a));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        int32_t deme = 0, ecap = 0, edone = 0;
        TRY(ppde_chains_annealing_shape(c, &deme, &ecap, &edone));
        if (ecap != 3 || edone != 3) { fprintf(stderr, "events %d of %d\n", edone, ecap); status = 92; goto done; }
        std::vector<int32_t> par((size_t)edone * n);
        std::vector<float> pre((size_t)edone * n), beta(n);
        std::vector<double> lmw((size_t)edone * (n / deme)), ess((size_t)edone * (n / deme));
        TRY(ppde_chains_annealing_read(c, 0, edone, par.data(), pre.data(), lmw.data(), ess.data(), beta.data()));
        TRY(ppde_chains_init(c, idx.data()));                                     // a second start
        TRY(ppde_chains_annealing_shape(c, nullptr, nullptr, &edone));
        if (edone != 0) { fprintf(stderr, "events after a second init: %d\n", edone); status = 91; goto done; }
    }
    {
        // what the shape of the object refuses: a shard that cuts a deme, two streams; and the queries without annealing
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 6; cfg.n_streams = 1;
        TRY(ppde_chains_create(&cs, m, &cfg));
        TRY(ppde_chains_set_reversible(cs, 1));
        ppde_anneal_config a4 = acfg(4, 1, 3, sched), a2 = acfg(2, 1, 3, sched);
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing(cs, &a4));          // chain_offset 6 is no multiple of 4
        TRY(ppde_chains_set_annealing(cs, &a2));                                   // ... but of 2
        cfg.chain_offset = 0; cfg.n_streams = 2;
        TRY(ppde_chains_create(&cn, m, &cfg));
        TRY(ppde_chains_set_reversible(cn, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_annealing(cn, &a4));          // two streams
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            std::vector<float> beta(n);
            EXPECT_INVALID(ppde_chains_annealing_shape(cn, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_annealing_read(cn, 0, 0, nullptr, nullptr, nullptr, nullptr, beta.data()));
        }
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
    return run_walks(argc, argv, "hostcheck anneal ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

// TEST INFRASTRUCTURE. Recombination's host side (ppde_chains_set_recombination, ppde_chains_recombination_shape / _read,
// include/ppde_hip.h) against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_library ->
// set_reversible -> set_recombination (every refusal, set / replace / clear, the calls blocked while it is set) -> init -> run ->
// recombination_shape / read -> collect -> destroy on both RNG modes and both gradient policies, an event-aligned and a misaligned
// run sequence over captured graphs, and -- with `driver sweep` -- the same walk once per fallible runtime call with that call
// failing, so every clean-up path runs. Kernels do not run here: numbers mean nothing, memory errors and leaks are the point.
// Besides the walks: the replay plan of ppde_chains_run (replay_plan below), with and without the mode.
#include "walk.h"

namespace {
ppde_recombine_config rcfg(int deme, int every) { ppde_recombine_config r{}; r.deme = deme; r.every = every; return r; }

int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cs = nullptr, *cn = nullptr;
    const int n = 8, T = 30, N = L * 20;
    const float sched[3] = {0.25f, 0.5f, 1.0f};
    const float ladder[2] = {1.0f, 0.5f};
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    std::vector<uint32_t> lib(L, 0u);
    int n_open = 0;
    for (int l = win; l < win + Lp; ++l)
        if (l % 3) { lib[l] = (1u << wt[l]) | (1u << ((wt[l] + 3) % 20)) | (1u << ((wt[l] + 7) % 20)); ++n_open; }
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
        // caller-supplied noise, trace on, a mutation cap: an event behind every second iteration, issued one iteration at a time
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        TRY(ppde_chains_set_library(c0, lib.data()));
        ppde_recombine_config good = rcfg(4, 2);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_recombination(c0, &good), "reversible");          // reversible mode not on
            EXPECT_INVALID(ppde_chains_recombination_shape(c0, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_set_reversible(c0, 1));
        if (refusals) {
            ppde_recombine_config r;
            EXPECT_INVALID(ppde_chains_set_recombination(nullptr, &good));
            r = rcfg(3, 2); EXPECT_INVALID(ppde_chains_set_recombination(c0, &r), "even");   // D odd
            r = rcfg(0, 2); EXPECT_INVALID(ppde_chains_set_recombination(c0, &r), "even");   // D < 2
            r = rcfg(6, 2); EXPECT_INVALID(ppde_chains_set_recombination(c0, &r), "n_chains");
            r = rcfg(4, 0); EXPECT_INVALID(ppde_chains_set_recombination(c0, &r), "every");
            r = rcfg(4, T + 1); EXPECT_INVALID(ppde_chains_set_recombination(c0, &r), "no event");   // events_cap == 0
            TRY(ppde_chains_set_tempering(c0, 2, ladder, 1));
            EXPECT_INVALID(ppde_chains_set_recombination(c0, &good), "tempering");
            TRY(ppde_chains_set_tempering(c0, 0, nullptr, 0));
            ppde_anneal_config an{}; an.deme = 4; an.every = 1; an.n_stages = 2; an.beta = sched;
            TRY(ppde_chains_set_annealing(c0, &an));
            EXPECT_INVALID(ppde_chains_set_recombination(c0, &good), "annealing");
            TRY(ppde_chains_set_annealing(c0, nullptr));
        }
        {
            ppde_recombine_config r = rcfg(2, T);                                 // the accepted edges, replaced below
            TRY(ppde_chains_set_recombination(c0, &r));
            r = rcfg(8, 1);
            TRY(ppde_chains_set_recombination(c0, &r));
        }
        TRY(ppde_chains_set_recombination(c0, nullptr));                          // cleared: the mode and the library are free again
        TRY(ppde_chains_set_reversible(c0, 0));
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_library(c0, lib.data()));
        TRY(ppde_chains_set_recombination(c0, &good));
        if (refusals) {
            ppde_anneal_config an{}; an.deme = 4; an.every = 1; an.n_stages = 2; an.beta = sched;
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 0), "recombination");   // the four calls blocked while it is set
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, ladder, 1), "recombination");
            EXPECT_INVALID(ppde_chains_set_annealing(c0, &an), "recombination");
            EXPECT_INVALID(ppde_chains_set_library(c0, lib.data()), "recombination");
            EXPECT_INVALID(ppde_chains_set_library(c0, nullptr), "recombination");
            std::vector<int32_t> par(n);
            EXPECT_INVALID(ppde_chains_recombination_read(c0, 0, 0, par.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));   // before init
            EXPECT_INVALID(ppde_chains_recombination_shape(c0, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_recombination(c0, &good), "before ppde_chains_init");   // after init
            EXPECT_INVALID(ppde_chains_set_recombination(c0, nullptr));
        }
        const int steps = 5;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        int32_t deme = 0, no = 0, cap = 0, done_ev = 0;
        TRY(ppde_chains_recombination_shape(c0, &deme, &no, nullptr, &cap, &done_ev));
        TRY(ppde_chains_recombination_shape(c0, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (deme != 4 || no != n_open || cap != T / 2 || done_ev != 2) { fprintf(stderr, "recombination shape %d %d %d %d\n", deme, no, cap, done_ev); status = 94; goto done; }
        std::vector<int32_t> sites(no), par((size_t)done_ev * n), lo((size_t)done_ev * n), hi((size_t)done_ev * n), dif((size_t)done_ev * n),
            cd((size_t)done_ev * n), bs(n);
        std::vector<uint8_t> oc((size_t)done_ev * n), bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        std::vector<float> lr((size_t)done_ev * n), pre((size_t)done_ev * n), che((size_t)done_ev * n), be(n), bf(n),
            eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        TRY(ppde_chains_recombination_shape(c0, nullptr, nullptr, sites.data(), nullptr, nullptr));
        for (int k = 0, l = win; l < win + Lp; ++l)
            if (l % 3) { if (sites[k++] != l) { fprintf(stderr, "open list\n"); status = 93; goto done; } }
        TRY(ppde_chains_recombination_read(c0, 0, done_ev, par.data(), lo.data(), hi.data(), dif.data(), cd.data(), oc.data(), lr.data(), pre.data(), che.data()));
        TRY(ppde_chains_recombination_read(c0, 1, 1, par.data(), nullptr, nullptr, nullptr, nullptr, oc.data(), nullptr, nullptr, che.data()));
        TRY(ppde_chains_recombination_read(c0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_recombination_read(c0, 0, done_ev + 1, par.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "beyond");
            EXPECT_INVALID(ppde_chains_recombination_read(c0, -1, 1, par.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recombination_read(c0, 2, 1, par.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        if (ppde_chains_steps_done(c0) != steps) { fprintf(stderr, "steps_done\n"); status = 97; goto done; }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG, graphs captured at init: every = 10 (segments of 100 -- too long for these histories -- and 10) run aligned,
        // every = 7 (98 is too long as well: segments of 7) entered at a misaligned position; the second object runs WITHOUT a library
        const int every = reuse ? 7 : 10;
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = reuse ? 2 : -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 104;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        if (!reuse) TRY(ppde_chains_set_library(c, lib.data()));
        TRY(ppde_chains_set_reversible(c, 1));
        ppde_recombine_config r = rcfg(reuse ? n : 2, every);
        TRY(ppde_chains_set_recombination(c, &r));
        TRY(ppde_chains_init(c, idx.data()));
        long long want_rep;
        if (!reuse) {                                                             // 20 + 10 + 7: 2 x 10, 10, nothing
            TRY(ppde_chains_run(c, 20, nullptr, nullptr, nullptr, nullptr));
            TRY(ppde_chains_run(c, 10, nullptr, nullptr, nullptr, nullptr));
            TRY(ppde_chains_run(c, 7, nullptr, nullptr, nullptr, nullptr));
            want_rep = 30;
        } else {                                                                  // 3 + 30 + 4: eager 3; eager 4, 3 x 7 replayed, eager 5; eager 2, 2 left eager
            TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
            TRY(ppde_chains_run(c, 30, nullptr, nullptr, nullptr, nullptr));
            TRY(ppde_chains_run(c, 4, nullptr, nullptr, nullptr, nullptr));
            want_rep = 21;
        }
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep != want_rep || rep + eag != 37 || cap != 1) {
            fprintf(stderr, "graph stats: %d captures (%d in run), %lld + %lld steps\n", cap, cap_run, (long long)rep, (long long)eag); status = 96; goto done;
        }
        int32_t deme = 0, no = 0, ecap = 0, edone = 0;
        TRY(ppde_chains_recombination_shape(c, &deme, &no, nullptr, &ecap, &edone));
        if (ecap != 2 * T / every || edone != 37 / every || no != (reuse ? L : n_open)) { fprintf(stderr, "events %d of %d, %d open\n", edone, ecap, no); status = 92; goto done; }
        std::vector<int32_t> par((size_t)edone * n);
        std::vector<float> pre((size_t)edone * n);
        std::vector<uint8_t> oc((size_t)edone * n);
        TRY(ppde_chains_recombination_read(c, 0, edone, par.data(), nullptr, nullptr, nullptr, nullptr, oc.data(), nullptr, pre.data(), nullptr));
        TRY(ppde_chains_init(c, idx.data()));                                     // a second start
        TRY(ppde_chains_recombination_shape(c, nullptr, nullptr, nullptr, nullptr, &edone));
        if (edone != 0) { fprintf(stderr, "events after a second init: %d\n", edone); status = 91; goto done; }
    }
    {
        // what the shape of the object refuses: a shard that cuts a deme, two streams; and the queries without the mode
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 6; cfg.n_streams = 1;
        TRY(ppde_chains_create(&cs, m, &cfg));
        TRY(ppde_chains_set_reversible(cs, 1));
        ppde_recombine_config r4 = rcfg(4, 1), r2 = rcfg(2, 1);
        if (refusals) EXPECT_INVALID(ppde_chains_set_recombination(cs, &r4), "chain_offset");   // chain_offset 6 is no multiple of 4
        TRY(ppde_chains_set_recombination(cs, &r2));                                            // ... but of 2
        cfg.chain_offset = 0; cfg.n_streams = 2;
        TRY(ppde_chains_create(&cn, m, &cfg));
        TRY(ppde_chains_set_reversible(cn, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_recombination(cn, &r4), "n_streams");      // two streams
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_recombination_shape(cn, nullptr, nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recombination_read(cn, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
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

// The replay plan: which iterations of a run are replayed from the graph segments captured at init and which are enqueued eagerly.
// Device RNG, use_graph, max_steps 130, runs of 7, 100 and 23 iterations; ppde_chains_graph_stats after each. Segments are taken
// longest first and, with recombination, start at multiples of `every` only:
//   no recombination (segments 100, 20): eager 7 | 100 | 20 + eager 3
//   every = 3 (segments 99, 3):          3 3 + eager 1 | eager 2, 32 x 3, eager 2 | eager 1, 7 x 3, eager 1
//   every = 7 (segments 98, 7):          7 | 98 + eager 2 | eager 5, 7 7, eager 4
// Nothing is captured inside a run.
int replay_plan(bool verbose) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains* c = nullptr;
    const int L = 48, Lp = 40, win = 4, n = 8;
    const int runs[3] = {7, 100, 23};
    struct Case { int every, captures; long long replayed[3], eager[3]; };
    const Case cases[3] = {{0, 2, {0, 100, 120}, {7, 7, 10}}, {3, 2, {6, 102, 123}, {1, 5, 7}}, {7, 2, {7, 105, 119}, {0, 2, 11}}};
    std::vector<uint8_t> wt(L, 3), idx((size_t)n * L, 3);
    auto J = rnd((size_t)Lp * Lp * 400, 0.05f), h = rnd((size_t)Lp * 20, 0.5f);
    TRY(ppde_model_create(&m, 0, L, wt.data()));
    TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));
    for (const Case& k : cases) {
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 130; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 3;
        TRY(ppde_chains_create(&c, m, &cfg));
        if (k.every) {
            ppde_recombine_config r = rcfg(2, k.every);
            TRY(ppde_chains_set_reversible(c, 1));
            TRY(ppde_chains_set_recombination(c, &r));
        }
        TRY(ppde_chains_init(c, idx.data()));
        for (int i = 0; i < 3; ++i) {
            TRY(ppde_chains_run(c, runs[i], nullptr, nullptr, nullptr, nullptr));
            int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
            TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
            if (verbose) fprintf(stderr, "replay plan, every = %d, after run %d: %d captures (%d in a run), %lld replayed, %lld eager\n", k.every, i,
                                 cap, cap_run, (long long)rep, (long long)eag);
            if (cap != k.captures || cap_run != 0 || rep != k.replayed[i] || eag != k.eager[i]) {
                fprintf(stderr, "replay plan, every = %d, run %d: expected %d captures (0 in a run), %lld replayed, %lld eager\n", k.every, i,
                        k.captures, k.replayed[i], k.eager[i]);
                status = 90; goto done;
            }
        }
        TRY(ppde_chains_sync(c));
        ppde_chains_destroy(c); c = nullptr;
    }
done:
    if (c) ppde_chains_destroy(c);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck recombine ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk, replay_plan);
}

// TEST INFRASTRUCTURE. The move statistics' host side (ppde_chains_set_stats, ppde_chains_stats_shape / _read, include/ppde_hip.h)
// against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: every refusal, then set -> replace -> clear ->
// set -> shape -> init -> read -> run -> read -> a second init -> destroy, on caller-supplied noise and on the device RNG (eager and
// from captured graphs, with a ladder, next to a recorder, pair counts and an archive set before and after them), and statistics that
// are never initialised; and -- with `driver sweep` -- the same walk once per fallible runtime call with that call failing, so
// every clean-up path runs.
// Kernels do not run here: numbers mean nothing beyond the zeros the fills wrote; memory errors and leaks are the point.
#include "walk.h"

namespace {
// host buffers of one read, sized by the shape the object reports
struct Out {
    std::vector<int64_t> chain[6], len[2], site;
    Out(int n, int R, int M, int L) { for (auto& v : chain) v.assign((size_t)n * R, -1); for (auto& v : len) v.assign((size_t)R * M, -1); site.assign((size_t)R * L, -1); }
};

#define EXPECT_SHAPE(c, R, M, S) do { int32_t r_ = -1, m_ = -1, s_ = -1; TRY(ppde_chains_stats_shape(c, &r_, &m_, &s_)); \
    if (r_ != (R) || m_ != (M) || s_ != (S)) { fprintf(stderr, "line %d: stats shape (%d, %d, %d), expected (%d, %d, %d)\n", __LINE__, r_, m_, s_, (int)(R), (int)(M), (int)(S)); status = 97; goto done; } } while (0)
#define READ_ALL(c, o) ppde_chains_stats_read(c, (o).chain[0].data(), (o).chain[1].data(), (o).chain[2].data(), (o).chain[3].data(), \
                                              (o).chain[4].data(), (o).chain[5].data(), (o).len[0].data(), (o).len[1].data(), (o).site.data())
#define READ_NO_SITES(c, o) ppde_chains_stats_read(c, (o).chain[0].data(), (o).chain[1].data(), (o).chain[2].data(), (o).chain[3].data(), \
                                                   (o).chain[4].data(), (o).chain[5].data(), (o).len[0].data(), (o).len[1].data(), nullptr)
#define READ_NONE(c) ppde_chains_stats_read(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)

bool all_zero(const Out& o, bool sites) {
    for (auto& v : o.chain) for (auto x : v) if (x) return false;
    for (auto& v : o.len) for (auto x : v) if (x) return false;
    if (sites) for (auto x : o.site) if (x) return false;
    return true;
}

// the walk; returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer)
int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cn = nullptr, *ce = nullptr;
    const int n = 8, T = 30, N = L * 20;
    const float ladder[4] = {1.0f, 0.5f, 0.25f, 0.125f};
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
        // default mode with paper_results on caller-supplied noise: every refusal, then statistics with per-site counts
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1; cfg.paper_results = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        ppde_stats_config a; a.per_site = 1;
        ppde_stats_config z; z.per_site = 0;
        Out o(n, 1, 3, L);
        if (refusals) {
            ppde_stats_config b;
            EXPECT_INVALID(ppde_chains_set_stats(nullptr, &a), "null");
            EXPECT_INVALID(ppde_chains_stats_shape(c0, nullptr, nullptr, nullptr), "no statistics were set");   // none yet
            EXPECT_INVALID(ppde_chains_stats_shape(nullptr, nullptr, nullptr, nullptr), "null");
            EXPECT_INVALID(READ_NONE(c0), "no statistics were set");
            EXPECT_INVALID(READ_NONE(nullptr), "no statistics were set");
            b.per_site = 2; EXPECT_INVALID(ppde_chains_set_stats(c0, &b), "per_site must be 0 or 1");
            b.per_site = -1; EXPECT_INVALID(ppde_chains_set_stats(c0, &b), "per_site must be 0 or 1");
            EXPECT_INVALID(ppde_chains_stats_shape(c0, nullptr, nullptr, nullptr), "no statistics were set");   // every refusal left the object unchanged
        }
        TRY(ppde_chains_set_stats(c0, &z)); EXPECT_SHAPE(c0, 1, 3, 0);
        TRY(ppde_chains_set_stats(c0, &a)); EXPECT_SHAPE(c0, 1, 3, 1);                          // replaced
        if (refusals) { ppde_stats_config b; b.per_site = 7; EXPECT_INVALID(ppde_chains_set_stats(c0, &b), "per_site must be 0 or 1"); EXPECT_SHAPE(c0, 1, 3, 1); }
        TRY(ppde_chains_set_stats(c0, nullptr));                                                // cleared, twice, then the one the run uses
        TRY(ppde_chains_set_stats(c0, nullptr));
        if (refusals) EXPECT_INVALID(ppde_chains_stats_shape(c0, nullptr, nullptr, nullptr), "no statistics were set");
        TRY(ppde_chains_set_stats(c0, &a));
        TRY(ppde_chains_set_stats(c0, &a));                                                     // replaced by itself
        EXPECT_SHAPE(c0, 1, 3, 1);
        TRY(ppde_chains_stats_shape(c0, nullptr, nullptr, nullptr));
        if (refusals) EXPECT_INVALID(READ_NONE(c0), "not initialised");                          // before init
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_stats(c0, &a), "before ppde_chains_init");             // after init: the graphs hold the pointers
            EXPECT_INVALID(ppde_chains_set_stats(c0, nullptr), "before ppde_chains_init");
        }
        TRY(READ_ALL(c0, o));                                                                   // before any run: zeros
        if (!all_zero(o, true)) { fprintf(stderr, "counters are not zero after init\n"); status = 96; goto done; }
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        mu[1] = 2; U[(size_t)1 * n] = 2;                                                        // an iteration whose noise covers two sub-steps
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        EXPECT_SHAPE(c0, 1, 3, 1);
        TRY(READ_ALL(c0, o));
        TRY(READ_NO_SITES(c0, o));
        TRY(ppde_chains_stats_read(c0, nullptr, o.chain[1].data(), nullptr, nullptr, nullptr, nullptr, nullptr, o.len[1].data(), nullptr));
        TRY(ppde_chains_stats_read(c0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, o.site.data()));
        TRY(READ_NONE(c0));
        TRY(ppde_chains_init(c0, idx.data()));                                                  // a second init, then on
        TRY(READ_ALL(c0, o));
        if (!all_zero(o, true)) { fprintf(stderr, "counters are not zero after a second init\n"); status = 96; goto done; }
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(READ_ALL(c0, o));
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold the statistics' kernels), replayed, then an eager remainder. The first object
        // has a ladder and the other observers set BEFORE the statistics; the second has no ladder, no per-site counts and sets them AFTER
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        ppde_stats_config a; a.per_site = reuse ? 0 : 1;
        ppde_archive_config ar; ar.k = 3;
        ppde_record_config r; r.burn_in = 3; r.every = 4; r.rung = -1; r.keep_samples = 1;
        ppde_pair_config p; p.n_sites = 0; p.sites = nullptr;
        const int R = reuse ? 1 : 4;
        if (!reuse) {
            TRY(ppde_chains_set_library(c, lib.data()));
            TRY(ppde_chains_set_reversible(c, 1));
            TRY(ppde_chains_set_stats(c, &a));                                                  // before the ladder: one rung ...
            EXPECT_SHAPE(c, 1, 5, 1);
            if (refusals) EXPECT_INVALID(ppde_chains_set_tempering(c, 4, ladder, 2), "move statistics are set");
            TRY(ppde_chains_set_stats(c, nullptr));
            TRY(ppde_chains_set_tempering(c, 4, ladder, 2));
            TRY(ppde_chains_set_recorder(c, &r));
            TRY(ppde_chains_set_pair_counts(c, &p));
            TRY(ppde_chains_set_archive(c, &ar));
            TRY(ppde_chains_set_stats(c, &a));                                                  // ... after it: the ladder's
            if (refusals) {
                EXPECT_INVALID(ppde_chains_set_tempering(c, 0, nullptr, 0), "move statistics are set");   // to clear
                EXPECT_INVALID(ppde_chains_set_tempering(c, 2, ladder, 1), "move statistics are set");    // to replace
                EXPECT_SHAPE(c, 4, 5, 1);
            }
        } else {
            TRY(ppde_chains_set_stats(c, &a));
            TRY(ppde_chains_set_recorder(c, &r));
            TRY(ppde_chains_set_pair_counts(c, &p));
            TRY(ppde_chains_set_archive(c, &ar));
            TRY(ppde_chains_set_stats(c, nullptr));                                             // independent of the other three: cleared and set again
            TRY(ppde_chains_set_stats(c, &a));
        }
        EXPECT_SHAPE(c, R, 5, a.per_site);
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 24, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30 || rep != 20) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        Out o(n, R, 5, L);
        if (a.per_site) TRY(READ_ALL(c, o));
        else {
            TRY(READ_NO_SITES(c, o));
            if (refusals) EXPECT_INVALID(READ_ALL(c, o), "per_site = 0");                        // site_changes that were never kept
        }
        for (auto x : o.chain[0]) if (x != 0) { fprintf(stderr, "a counter moved on a runtime that runs no kernel\n"); status = 96; goto done; }
        int32_t rows = 0, k = 0;
        TRY(ppde_chains_recorder_shape(c, &rows, nullptr, nullptr));
        TRY(ppde_chains_archive_shape(c, &k));
        if (rows != (30 - 3) / 4 || k != 3) { fprintf(stderr, "recorder rows %d, archive k %d next to statistics\n", rows, k); status = 96; goto done; }
        std::vector<uint64_t> pc((size_t)L * 20 * L * 20);
        TRY(ppde_chains_pair_counts_read(c, pc.data()));
    }
    {
        // what the shape of the object refuses: two streams; a run without statistics; and statistics on an object that is never initialised
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 0; cfg.n_streams = 2;
        ppde_stats_config a; a.per_site = 1;
        TRY(ppde_chains_create(&cn, m, &cfg));
        if (refusals) EXPECT_INVALID(ppde_chains_set_stats(cn, &a), "n_streams > 1");
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_stats_shape(cn, nullptr, nullptr, nullptr), "no statistics were set");
            EXPECT_INVALID(READ_NONE(cn), "no statistics were set");
        }
        TRY(ppde_chains_run(cn, 5, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(cn));
        cfg.n_streams = 1;
        TRY(ppde_chains_create(&ce, m, &cfg));
        TRY(ppde_chains_set_stats(ce, &a));                                                     // destroyed with its buffers, never run
    }
done:
    if (cn) ppde_chains_destroy(cn);
    if (ce) ppde_chains_destroy(ce);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}

// a run without statistics enqueues nothing new: the launches of 25 eager iterations with statistics exceed those without by
// exactly one per iteration, with per-site counts or without them
int launch_counts(bool verbose) {
    int status = PPDE_OK;
    const int L = 48, Lp = 40, win = 4, n = 8;
    ppde_model* m = nullptr;
    ppde_chains* c = nullptr;
    long base = -1;
    std::vector<uint8_t> wt(L, 3), idx((size_t)n * L, 3);
    TRY(ppde_model_create(&m, 0, L, wt.data()));
    {
        auto J = rnd((size_t)Lp * Lp * 400, 0.05f), h = rnd((size_t)Lp * 20, 0.5f);
        TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));
    }
    for (int mode = 0; mode < 3; ++mode) {                                                      // none, no sites, sites
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 30; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.reuse_grad = 1; cfg.random_chain = -1; cfg.use_graph = 0; cfg.n_streams = 1; cfg.seed = 3;
        TRY(ppde_chains_create(&c, m, &cfg));
        ppde_stats_config a; a.per_site = mode - 1;
        if (mode) TRY(ppde_chains_set_stats(c, &a));
        TRY(ppde_chains_init(c, idx.data()));
        const long l0 = hipmock_launches();
        TRY(ppde_chains_run(c, 25, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        const long got = hipmock_launches() - l0;
        if (mode == 0) base = got;
        else if (got != base + 25) { fprintf(stderr, "%ld launches with statistics (per_site %d), %ld without\n", got, mode - 1, base); status = 95; goto done; }
        ppde_chains_destroy(c); c = nullptr;
    }
done:
    if (c) ppde_chains_destroy(c);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck stats ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk, launch_counts);
}

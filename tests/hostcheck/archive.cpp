// TEST INFRASTRUCTURE. The archive's host side (ppde_chains_set_archive, ppde_chains_archive_shape / _read, include/ppde_hip.h)
// against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: every refusal, then set -> shape -> init ->
// run -> read -> a second init -> destroy, on caller-supplied noise and on the device RNG (eager and from captured graphs, with a
// ladder, next to a recorder and pair counts set before and after it), clearing, and an archive that is never initialised; and
// -- with `driver sweep` -- the same walk once per fallible runtime call with that call failing, so every clean-up path runs.
// Kernels do not run here: numbers mean nothing, memory errors and leaks are the point (and the fill of the empty slots, which is
// the host's).
#include "walk.h"

namespace {
#define EXPECT_K(c, want) do { int32_t k_ = -1; TRY(ppde_chains_archive_shape(c, &k_)); \
    if (k_ != (want)) { fprintf(stderr, "line %d: archive shape %d, expected %d\n", __LINE__, k_, (int)(want)); status = 97; goto done; } } while (0)

// the walk; returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer)
int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cn = nullptr, *cp = nullptr, *ce = nullptr;
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
        // default mode on caller-supplied noise: every refusal, then an archive of 5 entries per chain
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        ppde_archive_config a; a.k = 5;
        if (refusals) {
            ppde_archive_config b;
            EXPECT_INVALID(ppde_chains_set_archive(nullptr, &a), "null");
            EXPECT_INVALID(ppde_chains_archive_shape(c0, nullptr), "no archive was set");           // no archive yet
            EXPECT_INVALID(ppde_chains_archive_read(c0, nullptr, nullptr, nullptr, nullptr, nullptr), "no archive was set");
            b.k = 0; EXPECT_INVALID(ppde_chains_set_archive(c0, &b), "1..32");
            b.k = -1; EXPECT_INVALID(ppde_chains_set_archive(c0, &b), "1..32");
            b.k = 33; EXPECT_INVALID(ppde_chains_set_archive(c0, &b), "1..32");
            EXPECT_INVALID(ppde_chains_archive_shape(c0, nullptr), "no archive was set");           // every refusal left the object unchanged
        }
        { ppde_archive_config e; e.k = 1; TRY(ppde_chains_set_archive(c0, &e)); EXPECT_K(c0, 1); }
        { ppde_archive_config e; e.k = 32; TRY(ppde_chains_set_archive(c0, &e)); EXPECT_K(c0, 32); }   // replaced
        if (refusals) { ppde_archive_config b; b.k = 33; EXPECT_INVALID(ppde_chains_set_archive(c0, &b), "1..32"); EXPECT_K(c0, 32); }
        TRY(ppde_chains_set_archive(c0, nullptr));                                              // cleared, twice, then the one the run uses
        TRY(ppde_chains_set_archive(c0, nullptr));
        if (refusals) EXPECT_INVALID(ppde_chains_archive_shape(c0, nullptr), "no archive was set");
        TRY(ppde_chains_set_archive(c0, &a));
        TRY(ppde_chains_set_archive(c0, &a));                                                   // replaced by itself
        EXPECT_K(c0, 5);
        if (refusals) EXPECT_INVALID(ppde_chains_archive_read(c0, nullptr, nullptr, nullptr, nullptr, nullptr), "not initialised");
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_archive(c0, &a), "before ppde_chains_init");           // after init: the graphs hold the pointers
            EXPECT_INVALID(ppde_chains_set_archive(c0, nullptr), "before ppde_chains_init");
        }
        std::vector<uint8_t> ai((size_t)n * 5 * L);
        std::vector<float> ae((size_t)n * 5), af((size_t)n * 5);
        std::vector<int32_t> as((size_t)n * 5), ac(n);
        TRY(ppde_chains_archive_read(c0, ai.data(), ae.data(), af.data(), as.data(), ac.data()));   // before any run: row 0 only
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        EXPECT_K(c0, 5);
        TRY(ppde_chains_archive_read(c0, ai.data(), ae.data(), af.data(), as.data(), ac.data()));
        TRY(ppde_chains_archive_read(c0, nullptr, ae.data(), nullptr, as.data(), nullptr));
        TRY(ppde_chains_archive_read(c0, ai.data(), nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_archive_read(c0, nullptr, nullptr, nullptr, nullptr, nullptr));
        // the mock runs no kernel, so every count is the zero the fill wrote: the empty slots are the host's to fill
        for (int b = 0; b < n; ++b) {
            if (ac[b] != 0) { fprintf(stderr, "count[%d] = %d on a runtime that runs no kernel\n", b, ac[b]); status = 96; goto done; }
            for (int j = 0; j < 5; ++j) {
                const size_t o = (size_t)b * 5 + j;
                if (!(ae[o] == -INFINITY) || af[o] != 0.f || as[o] != -1 || ai[o * L] != 255 || ai[o * L + L - 1] != 255) {
                    fprintf(stderr, "empty slot (%d, %d) is not filled\n", b, j); status = 96; goto done; }
            }
        }
        TRY(ppde_chains_init(c0, idx.data()));                                                  // a second init, then on
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_archive_read(c0, ai.data(), ae.data(), af.data(), as.data(), ac.data()));
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold k_archive), replayed, then an eager remainder. The first object has a ladder
        // and a recorder with pair counts set BEFORE the archive; the second has no ladder and sets them AFTER it
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        ppde_archive_config a; a.k = reuse ? 32 : 3;
        ppde_record_config r; r.burn_in = 3; r.every = 4; r.rung = -1; r.keep_samples = 1;
        ppde_pair_config p; p.n_sites = 0; p.sites = nullptr;
        if (!reuse) {
            TRY(ppde_chains_set_library(c, lib.data()));
            TRY(ppde_chains_set_reversible(c, 1));
            TRY(ppde_chains_set_tempering(c, 4, ladder, 2));
            TRY(ppde_chains_set_recorder(c, &r));
            TRY(ppde_chains_set_pair_counts(c, &p));
            TRY(ppde_chains_set_archive(c, &a));
        } else {
            TRY(ppde_chains_set_archive(c, &a));
            TRY(ppde_chains_set_recorder(c, &r));
            TRY(ppde_chains_set_pair_counts(c, &p));
            TRY(ppde_chains_set_archive(c, nullptr));                                           // independent of the other two: cleared and set again
            TRY(ppde_chains_set_archive(c, &a));
        }
        EXPECT_K(c, a.k);
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 24, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30 || rep != 20) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        std::vector<uint8_t> ai((size_t)n * a.k * L);
        std::vector<float> ae((size_t)n * a.k), af((size_t)n * a.k);
        std::vector<int32_t> as((size_t)n * a.k), ac(n);
        TRY(ppde_chains_archive_read(c, ai.data(), ae.data(), af.data(), as.data(), ac.data()));
        int32_t rows = 0;
        TRY(ppde_chains_recorder_shape(c, &rows, nullptr, nullptr));
        if (rows != (30 - 3) / 4) { fprintf(stderr, "recorder rows %d next to an archive\n", rows); status = 96; goto done; }
        std::vector<uint64_t> pc((size_t)L * 20 * L * 20);
        TRY(ppde_chains_pair_counts_read(c, pc.data()));
    }
    {
        // what the shape of the object refuses: two streams, paper_results; and an archive on an object that is never initialised
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 0; cfg.n_streams = 2;
        ppde_archive_config a; a.k = 4;
        TRY(ppde_chains_create(&cn, m, &cfg));
        if (refusals) EXPECT_INVALID(ppde_chains_set_archive(cn, &a), "n_streams > 1");
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_archive_shape(cn, nullptr), "no archive was set");
            EXPECT_INVALID(ppde_chains_archive_read(cn, nullptr, nullptr, nullptr, nullptr, nullptr), "no archive was set");
        }
        TRY(ppde_chains_run(cn, 5, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(cn));
        cfg.n_streams = 1; cfg.paper_results = 1;
        TRY(ppde_chains_create(&cp, m, &cfg));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_archive(cp, &a), "paper_results");
            EXPECT_INVALID(ppde_chains_archive_shape(cp, nullptr), "no archive was set");
        }
        cfg.paper_results = 0;
        TRY(ppde_chains_create(&ce, m, &cfg));
        TRY(ppde_chains_set_archive(ce, &a));                                                   // destroyed with its buffers, never run
    }
done:
    if (cn) ppde_chains_destroy(cn);
    if (cp) ppde_chains_destroy(cp);
    if (ce) ppde_chains_destroy(ce);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck archive ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

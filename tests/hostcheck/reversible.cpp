// TEST INFRASTRUCTURE. Reversible mode's host side (ppde_chains_set_reversible, include/ppde_hip.h) against the mock runtime of
// tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_library -> set_reversible -> init -> run -> collect ->
// destroy on both RNG modes and both gradient policies (the separate and the fused accept kernels, eager and from captured
// graphs), the mode's refusals, and -- with `driver sweep` -- the same walk once per fallible runtime call with that call failing,
// so every clean-up path runs. Kernels do not run here: numbers mean nothing, memory errors and leaks are the point.
#include "walk.h"

namespace {
// the walk; returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer)
int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cp = nullptr;
    const int n = 6, T = 30, N = L * 20;
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    // a library over the window: every third residue frozen, the others with their wild-type letter and four more
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
        // caller-supplied noise (flat race), trace on, a mutation cap: k_accept_rev in its replay form
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        TRY(ppde_chains_set_library(c0, lib.data()));
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_reversible(c0, 0));                                   // off and on again before init: both fine
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 1));                    // after init: the graphs hold the kernel choice
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 0));
            EXPECT_INVALID(ppde_chains_set_reversible(nullptr, 1));
        }
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        std::vector<int32_t> flat((size_t)steps * 3 * n), Ut((size_t)steps * n), dist(n), bs(n);
        std::vector<uint8_t> acc((size_t)steps * n), pidx((size_t)n * L), pacc(n), bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        std::vector<float> la((size_t)steps * n), e(n), fit(n), be(n), bf(n), eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        TRY(ppde_chains_trace(c0, flat.data(), acc.data(), la.data(), Ut.data()));
        TRY(ppde_chains_peek(c0, pidx.data(), e.data(), fit.data(), pacc.data(), dist.data()));
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        if (ppde_chains_steps_done(c0) != steps) { fprintf(stderr, "steps_done\n"); status = 97; goto done; }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold the *_rev kernels), replayed, then an eager remainder; reuse = 1 goes
        // through the fused accept + propose kernel, on two streams; the second object runs WITHOUT a library
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1 + reuse; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        if (!reuse) TRY(ppde_chains_set_library(c, lib.data()));
        TRY(ppde_chains_set_reversible(c, 1));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        const int done_steps = ppde_chains_steps_done(c);
        std::vector<uint8_t> bi((size_t)n * L);
        std::vector<float> be(n), bf(n), eh((size_t)(done_steps + 1) * n), fh((size_t)(done_steps + 1) * n);
        std::vector<int32_t> bs(n);
        TRY(ppde_chains_collect(c, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), nullptr));
    }
    {
        // paper_results: the mode is refused, switching it off is not, and the object still runs as before
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.paper_results = 1; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5;
        TRY(ppde_chains_create(&cp, m, &cfg));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_reversible(cp, 1));
            if (!strstr(ppde_last_error(), "paper_results")) { fprintf(stderr, "the refusal does not name paper_results: %s\n", ppde_last_error()); status = 95; goto done; }
        }
        TRY(ppde_chains_set_reversible(cp, 0));
        TRY(ppde_chains_init(cp, idx.data()));
        TRY(ppde_chains_run(cp, 5, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(cp));
    }
done:
    if (cp) ppde_chains_destroy(cp);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck reversible ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

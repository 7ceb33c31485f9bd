// TEST INFRASTRUCTURE. Parallel tempering's host side (ppde_chains_set_tempering, ppde_chains_tempering_state / _history,
// include/ppde_hip.h) against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_library ->
// set_reversible -> set_tempering (every refusal, then a valid ladder) -> init -> run -> tempering_state / history -> collect ->
// destroy on both RNG modes and both gradient policies (eager and from captured graphs), and -- with `driver sweep` -- the same walk
// once per fallible runtime call with that call failing, so every clean-up path runs. Kernels do not run here: numbers mean
// nothing, memory errors and leaks are the point.
#include "walk.h"

namespace {
// the walk; returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer)
int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *cs = nullptr, *cn = nullptr;
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
        // caller-supplied noise (flat race), trace on, a mutation cap: the *_temp kernels in their replay form, a swap every iteration
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        TRY(ppde_chains_set_library(c0, lib.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 4, ladder, 1));           // reversible mode not on
            if (!strstr(ppde_last_error(), "reversible")) { fprintf(stderr, "the refusal does not name reversible mode: %s\n", ppde_last_error()); status = 95; goto done; }
        }
        TRY(ppde_chains_set_reversible(c0, 1));
        if (refusals) {
            std::vector<float> big(65);
            for (int r = 0; r < 65; ++r) big[r] = 2.0f - 0.01f * r;
            const float flat2[2] = {1.0f, 1.0f}, up[2] = {0.5f, 1.0f}, zero[2] = {1.0f, 0.0f}, neg[2] = {1.0f, -1.0f};
            const float nan2[2] = {1.0f, NAN}, inf2[2] = {INFINITY, 1.0f}, three[3] = {1.0f, 0.5f, 0.25f};
            EXPECT_INVALID(ppde_chains_set_tempering(nullptr, 4, ladder, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 65, big.data(), 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, -1, ladder, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, flat2, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, up, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, zero, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, neg, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, nan2, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 2, inf2, 1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 4, ladder, -1));
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 3, three, 1));            // 8 chains are no multiple of 3
        }
        TRY(ppde_chains_set_tempering(c0, 2, ladder, 3));
        TRY(ppde_chains_set_tempering(c0, 0, nullptr, 0));                        // cleared, then the ladder the run uses
        TRY(ppde_chains_set_reversible(c0, 0));                                   // (no tempering set: switching the mode off is fine)
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_tempering(c0, 4, ladder, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_reversible(c0, 0));          // tempering needs the mode
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 4, ladder, 1));           // after init: the graphs hold the kernel choice
            EXPECT_INVALID(ppde_chains_set_tempering(c0, 0, nullptr, 0));
        }
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        std::vector<int32_t> rung(n), bs(n);
        std::vector<float> beta(n), be(n), bf(n), eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        std::vector<int64_t> att((size_t)(n / 4) * 3), acc((size_t)(n / 4) * 3);
        std::vector<uint8_t> rh((size_t)(steps + 1) * n), bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        TRY(ppde_chains_tempering_state(c0, rung.data(), beta.data(), att.data(), acc.data()));
        TRY(ppde_chains_tempering_state(c0, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_tempering_history(c0, rh.data()));
        for (int b = 0; b < n; ++b)
            if (rung[b] != b % 4 || beta[b] != ladder[b % 4] || rh[b] != b % 4) { fprintf(stderr, "start rungs\n"); status = 94; goto done; }
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        if (ppde_chains_steps_done(c0) != steps) { fprintf(stderr, "steps_done\n"); status = 97; goto done; }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold the *_temp kernels and k_swap), replayed, then an eager remainder; the
        // second object runs WITHOUT a library, one rung and no exchange
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        if (!reuse) TRY(ppde_chains_set_library(c, lib.data()));
        TRY(ppde_chains_set_reversible(c, 1));
        TRY(ppde_chains_set_tempering(c, reuse ? 1 : 4, ladder, reuse ? 0 : 2));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        const int done_steps = ppde_chains_steps_done(c), R = reuse ? 1 : 4;
        std::vector<int32_t> rung(n);
        std::vector<float> beta(n);
        std::vector<int64_t> att((size_t)(n / R) * (R - 1)), acc((size_t)(n / R) * (R - 1));
        std::vector<uint8_t> rh((size_t)(done_steps + 1) * n);
        TRY(ppde_chains_tempering_state(c, rung.data(), beta.data(), att.data(), acc.data()));
        TRY(ppde_chains_tempering_history(c, rh.data()));
    }
    {
        // what the shape of the object refuses: a shard that cuts an ensemble, two streams; and the queries without tempering
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 6; cfg.n_streams = 1;
        TRY(ppde_chains_create(&cs, m, &cfg));
        TRY(ppde_chains_set_reversible(cs, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_tempering(cs, 4, ladder, 1));   // chain_offset 6 is no multiple of 4
        TRY(ppde_chains_set_tempering(cs, 2, ladder, 1));                           // ... but of 2
        cfg.chain_offset = 0; cfg.n_streams = 2;
        TRY(ppde_chains_create(&cn, m, &cfg));
        TRY(ppde_chains_set_reversible(cn, 1));
        if (refusals) EXPECT_INVALID(ppde_chains_set_tempering(cn, 4, ladder, 1));   // two streams
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            std::vector<uint8_t> rh((size_t)n);
            EXPECT_INVALID(ppde_chains_tempering_state(cn, nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_tempering_history(cn, rh.data()));
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
    return run_walks(argc, argv, "hostcheck tempering ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

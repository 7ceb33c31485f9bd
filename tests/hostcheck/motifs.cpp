// TEST INFRASTRUCTURE. The forbidden patterns' host side (ppde_chains_set_forbidden_patterns, ppde_chains_forbidden_shape / _read,
// ppde_motif_scan, include/ppde_hip.h) against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create ->
// set_reversible -> set_forbidden_patterns (every refusal, set / replace / clear, set_reversible(0) blocked while it is set) -> init
// -> run -> forbidden_shape / read -> collect -> destroy on both RNG modes, both gradient policies, one and two streams and next
// to recombination, and -- with `driver sweep` -- the same walk once per fallible runtime call with that call failing, so every
// clean-up path runs. Kernels do not run here: numbers mean nothing, memory errors and leaks are the point.
#include "walk.h"

namespace {
struct Pats {
    std::vector<int32_t> len;
    std::vector<uint32_t> el;
    ppde_motif_config cfg{};
    Pats(int M, int length, uint32_t word, int allow_native = 1) : len(M > 0 ? M : 1, length), el((size_t)(M > 0 ? M : 1) * 8, word) {
        cfg.n_patterns = M; cfg.length = len.data(); cfg.element = el.data(); cfg.allow_native = allow_native;
    }
};

int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr;
    const int n = 8, T = 30, N = L * 20;
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    // a pair the wild type holds at 0 (native) and two letter classes
    const uint32_t other = 0xfffffu & ~(1u << wt[0]);
    Pats good(3, 2, 0x00f0fu), full(32, 8, 0xfffffu & ~(1u << wt[3])), strict(1, 1, 1u << wt[0], 0);
    good.el[0] = 1u << wt[0]; good.el[1] = 1u << wt[1];
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
        // caller-supplied noise, trace on, a mutation cap
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        std::vector<uint32_t> act(L);
        int32_t M = 0, an = -1;
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &good.cfg), "reversible");  // reversible mode not on
            EXPECT_INVALID(ppde_chains_forbidden_shape(c0, &M, &an, act.data()), "no patterns");
        }
        TRY(ppde_chains_set_reversible(c0, 1));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_forbidden_patterns(nullptr, &good.cfg));
            { Pats p(0, 1, 1u); EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "1..32"); }
            { Pats p(33, 1, other); EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "1..32"); }
            { Pats p(2, 1, other); p.len[1] = 0; EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "pattern 1: length"); }
            { Pats p(2, 1, other); p.len[0] = 9; EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "pattern 0: length"); }
            { Pats p(2, 2, other); p.el[8 + 1] = 0u; EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "pattern 1, element 1: empty"); }
            { Pats p(2, 2, other); p.el[0] = 1u << 20; EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "pattern 0, element 0: a bit >= 20"); }
            { Pats p(1, 1, 0xfffffu); EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "no active"); }   // the wild type matches everywhere
            { Pats p(1, 1, other); p.cfg.length = nullptr; EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &p.cfg), "null"); }
        }
        { Pats p(2, 1, other); p.el[1] = 1u << 20; p.el[8 + 7] = 0u; TRY(ppde_chains_set_forbidden_patterns(c0, &p.cfg)); }   // words behind a length are ignored
        TRY(ppde_chains_set_forbidden_patterns(c0, &full.cfg));                     // replaced: the edges M = 32, length 8
        TRY(ppde_chains_forbidden_shape(c0, &M, &an, act.data()));
        if (M != 32 || an != 1 || act[0] != 0xffffffffu || act[L - 7] != 0u) { fprintf(stderr, "shape %d %d %x\n", M, an, act[0]); status = 94; goto done; }
        TRY(ppde_chains_set_forbidden_patterns(c0, nullptr));                       // cleared: reversible mode is free again
        TRY(ppde_chains_set_reversible(c0, 0));
        TRY(ppde_chains_set_reversible(c0, 1));
        TRY(ppde_chains_set_forbidden_patterns(c0, &strict.cfg));                   // allow_native 0 and a wild type that matches: legal, with a note
        if (!strstr(ppde_last_error(), "note: the wild type matches pattern 0 at position 0")) { fprintf(stderr, "no note: %s\n", ppde_last_error()); status = 93; goto done; }
        TRY(ppde_chains_set_forbidden_patterns(c0, &good.cfg));
        if (ppde_last_error()[0]) { fprintf(stderr, "a stale note: %s\n", ppde_last_error()); status = 92; goto done; }
        TRY(ppde_chains_forbidden_shape(c0, &M, &an, act.data()));
        if (M != 3 || (act[0] & 1u) || !(act[1] & 1u) || act[L - 1] != 0u) { fprintf(stderr, "active %x %x\n", act[0], act[1]); status = 91; goto done; }
        std::vector<int64_t> vt((size_t)n * 3);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_reversible(c0, 0), "pattern constraint");   // blocked while it is set
            EXPECT_INVALID(ppde_chains_forbidden_read(c0, vt.data()), "not initialised");
        }
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, &good.cfg), "before ppde_chains_init");
            EXPECT_INVALID(ppde_chains_set_forbidden_patterns(c0, nullptr));
        }
        const int steps = 5;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        TRY(ppde_chains_forbidden_read(c0, vt.data()));
        TRY(ppde_chains_forbidden_read(c0, nullptr));
        std::vector<int32_t> bs(n);
        std::vector<uint8_t> bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        std::vector<float> be(n), bf(n), eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        // the scan on its own: the mock's "device" rows are host memory
        std::vector<int32_t> fp(n, 7), fq(n, 7);
        TRY(ppde_motif_scan(m, &good.cfg, idx.data(), n, fp.data(), fq.data(), nullptr));
        if (refusals) {
            Pats p(0, 1, 1u);
            EXPECT_INVALID(ppde_motif_scan(m, &p.cfg, idx.data(), n, fp.data(), fq.data(), nullptr), "1..32");
            EXPECT_INVALID(ppde_motif_scan(m, &good.cfg, idx.data(), 0, fp.data(), fq.data(), nullptr), "at least one row");
            EXPECT_INVALID(ppde_motif_scan(m, &good.cfg, nullptr, n, fp.data(), fq.data(), nullptr));
        }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG, graphs captured at init; two streams without recombination, one with it (an event every 10 iterations)
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = reuse ? 2 : -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = reuse ? 2 : 1; cfg.seed = 11; cfg.chain_offset = 104;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        TRY(ppde_chains_set_reversible(c, 1));
        TRY(ppde_chains_set_forbidden_patterns(c, &good.cfg));
        if (!reuse) { ppde_recombine_config r{}; r.deme = 4; r.every = 10; TRY(ppde_chains_set_recombination(c, &r)); }
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 20, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 17, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 37 || rep < 20) { fprintf(stderr, "graph stats: %d captures (%d in run), %lld + %lld steps\n", cap, cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        std::vector<int64_t> vt((size_t)n * 3, -1);
        TRY(ppde_chains_forbidden_read(c, vt.data()));
        TRY(ppde_chains_init(c, idx.data()));                                       // a second start zeroes the counters
        TRY(ppde_chains_forbidden_read(c, vt.data()));
        for (int64_t v : vt) if (v != 0) { fprintf(stderr, "counters after a second init\n"); status = 95; goto done; }
    }
done:
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck motifs ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

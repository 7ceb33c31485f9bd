// TEST INFRASTRUCTURE. The host side of the pair counts (ppde_chains_set_pair_counts, ppde_chains_pair_counts_shape / _read,
// include/ppde_hip.h) against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: every refusal, then a
// valid set -> shape -> init -> run -> read -> (a second init) -> destroy, with all residues and with a ragged site list, on
// caller-supplied noise and on the device RNG (eager and from captured graphs), with a ladder and a rung recorder; clear, replace,
// and an object destroyed without ever being initialised; and -- with `driver sweep` -- the same walk once per fallible runtime
// call with that call failing, so every clean-up path runs. Kernels do not run here: the counts are zero, memory errors and leaks
// are the point (and the unpacking of the tile blocks into the full symmetric array, which is the host's).
#include "walk.h"

namespace {
#define EXPECT_SITES(c, want) do { int32_t s_ = -1; TRY(ppde_chains_pair_counts_shape(c, &s_, nullptr)); \
    std::vector<int32_t> got_((size_t)(s_ > 0 ? s_ : 0), -7); TRY(ppde_chains_pair_counts_shape(c, nullptr, got_.data())); \
    if (got_ != (want)) { fprintf(stderr, "line %d: pair sites differ (%d sites, expected %d)\n", __LINE__, (int)s_, (int)(want).size()); \
        status = 97; goto done; } } while (0)
#define EXPECT_MESSAGE(word) do { if (!strstr(ppde_last_error(), word)) { \
    fprintf(stderr, "line %d: the refusal does not say \"%s\": %s\n", __LINE__, word, ppde_last_error()); status = 95; goto done; } } while (0)

ppde_record_config rc_of(int burn_in, int every, int rung, int keep) {
    ppde_record_config r;
    r.burn_in = burn_in; r.every = every; r.rung = rung; r.keep_samples = keep;
    return r;
}
ppde_pair_config pc_of(const std::vector<int32_t>& s) {
    ppde_pair_config p;
    p.n_sites = (int32_t)s.size(); p.sites = s.empty() ? nullptr : s.data();
    return p;
}

int walk(int L, int Lp, int win, bool verbose, bool refusals) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *ce = nullptr;
    const int n = 8, T = 30, N = L * 20;
    const float ladder[4] = {1.0f, 0.5f, 0.25f, 0.125f};
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (int b = 0; b < n; ++b) for (int l = 0; l < L; ++l) idx[(size_t)b * L + l] = wt[l];
    std::vector<uint32_t> lib(L, 0u);
    for (int l = win; l < win + Lp; ++l)
        if (l % 3) lib[l] = (1u << wt[l]) | (1u << ((wt[l] + 3) % 20)) | (1u << ((wt[l] + 7) % 20));
    std::vector<int32_t> all(L), ragged = {0, 3, 4, L / 2, L - 1}, one = {L - 1};      // 5 sites: two tiles per side, the last ragged
    for (int l = 0; l < L; ++l) all[l] = l;
    const ppde_pair_config every_residue = pc_of({}), p_ragged = pc_of(ragged), p_one = pc_of(one);
    TRY(ppde_model_create(&m, 0, L, wt.data()));
    {
        auto J = rnd((size_t)Lp * Lp * 400, 0.05f), h = rnd((size_t)Lp * 20, 0.5f);
        TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));
    }
    {
        // default mode on caller-supplied noise: every refusal, then pair counts over every residue
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        ppde_record_config r = rc_of(0, 1, -1, 1);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_pair_counts(nullptr, &every_residue));
            EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &every_residue));                    // no recorder
            EXPECT_MESSAGE("no recorder");
            EXPECT_INVALID(ppde_chains_pair_counts_shape(c0, nullptr, nullptr));                // no pair counts
            EXPECT_INVALID(ppde_chains_pair_counts_shape(nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_set_pair_counts(c0, nullptr));                                          // clearing nothing is fine
        TRY(ppde_chains_set_recorder(c0, &r));
        if (refusals) {
            std::vector<int32_t> s;
            ppde_pair_config b;
            b.n_sites = -1; b.sites = nullptr; EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b));
            b.n_sites = -1; b.sites = all.data(); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b));
            std::vector<int32_t> too_many(L + 1, 0);
            b.n_sites = L + 1; b.sites = too_many.data(); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b));
            b.n_sites = 2; b.sites = nullptr; EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b));
            b.n_sites = 0; b.sites = all.data(); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b));
            s = {-1, 2}; b = pc_of(s); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b)); EXPECT_MESSAGE("outside");
            s = {0, L}; b = pc_of(s); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b)); EXPECT_MESSAGE("outside");
            s = {1, 1}; b = pc_of(s); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b)); EXPECT_MESSAGE("strictly increasing");
            s = {0, 5, 4}; b = pc_of(s); EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &b)); EXPECT_MESSAGE("strictly increasing");
            EXPECT_INVALID(ppde_chains_pair_counts_shape(c0, nullptr, nullptr));                // every refusal left the object unchanged
        }
        TRY(ppde_chains_set_pair_counts(c0, &p_one));
        EXPECT_SITES(c0, one);
        TRY(ppde_chains_set_pair_counts(c0, &p_ragged));                                        // replaced
        EXPECT_SITES(c0, ragged);
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_recorder(c0, nullptr));                               // neither cleared ...
            EXPECT_MESSAGE("clear the pair counts first");
            EXPECT_INVALID(ppde_chains_set_recorder(c0, &r));                                    // ... nor replaced
            EXPECT_MESSAGE("clear the pair counts first");
        }
        TRY(ppde_chains_set_pair_counts(c0, nullptr));
        if (refusals) EXPECT_INVALID(ppde_chains_pair_counts_shape(c0, nullptr, nullptr));
        TRY(ppde_chains_set_recorder(c0, &r));                                                  // without them the recorder may change again
        TRY(ppde_chains_set_pair_counts(c0, &every_residue));
        EXPECT_SITES(c0, all);
        std::vector<uint64_t> pc((size_t)L * 20 * L * 20, 1);
        if (refusals) EXPECT_INVALID(ppde_chains_pair_counts_read(c0, pc.data()));               // not initialised
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_pair_counts(c0, &every_residue));                     // after init: the graphs hold the pointers
            EXPECT_INVALID(ppde_chains_set_pair_counts(c0, nullptr));
            EXPECT_INVALID(ppde_chains_pair_counts_read(nullptr, pc.data()));
        }
        const int steps = 3;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_pair_counts_read(c0, pc.data()));                                       // synchronises; writes every entry
        for (uint64_t v : pc) if (v != 0) { fprintf(stderr, "read left an entry of the array unwritten\n"); status = 94; goto done; }
        TRY(ppde_chains_pair_counts_read(c0, nullptr));
        TRY(ppde_chains_init(c0, idx.data()));                                                  // a second start zeroes the counts
        TRY(ppde_chains_pair_counts_read(c0, pc.data()));
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold k_record_pairs), replayed, then an eager remainder. The first object
        // follows the last rung of a ladder; the second has no ladder and a counts-only recorder. Both with the ragged list
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        ppde_record_config r = rc_of(3, 4, reuse ? -1 : 3, reuse ? 0 : 1);
        if (!reuse) {
            TRY(ppde_chains_set_library(c, lib.data()));
            TRY(ppde_chains_set_reversible(c, 1));
            TRY(ppde_chains_set_tempering(c, 4, ladder, 2));
        }
        TRY(ppde_chains_set_recorder(c, &r));
        TRY(ppde_chains_set_pair_counts(c, &p_ragged));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        std::vector<uint64_t> pc((size_t)5 * 20 * 5 * 20, 1);
        TRY(ppde_chains_pair_counts_read(c, pc.data()));
        for (uint64_t v : pc) if (v != 0) { fprintf(stderr, "read left an entry of the ragged array unwritten\n"); status = 94; goto done; }
        std::vector<uint64_t> cnt((size_t)L * 20);
        TRY(ppde_chains_recorder_read(c, 0, 0, nullptr, nullptr, nullptr, nullptr, cnt.data()));
    }
    {
        // pair counts on an object that is never initialised: destroyed with their buffers
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.n_streams = 1;
        ppde_record_config r = rc_of(0, 1, -1, 0);
        TRY(ppde_chains_create(&ce, m, &cfg));
        TRY(ppde_chains_set_recorder(ce, &r));
        TRY(ppde_chains_set_pair_counts(ce, &every_residue));
    }
done:
    if (ce) ppde_chains_destroy(ce);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck pairs ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

// TEST INFRASTRUCTURE. The recorder's host side (ppde_chains_set_recorder, ppde_chains_recorder_shape / _read, include/ppde_hip.h)
// against the mock runtime of tests/hostcheck/ under AddressSanitizer + LeakSanitizer: create -> set_recorder (every refusal, then a
// valid one) -> init -> run -> shape -> read -> destroy, on caller-supplied noise, on the device RNG (eager and from captured
// graphs), with a ladder and a rung recorder, counts only, and at the edges of the row schedule; and -- with `driver sweep` -- the
// same walk once per fallible runtime call with that call failing, so every clean-up path runs. Kernels do not run here: numbers
// mean nothing, memory errors and leaks are the point (and the row arithmetic, which is the host's).
#include "walk.h"

namespace {
#define EXPECT_SHAPE(c, d, cap, sl) do { int32_t d_ = -1, c_ = -1, s_ = -1; TRY(ppde_chains_recorder_shape(c, &d_, &c_, &s_)); \
    if (d_ != (d) || c_ != (cap) || s_ != (sl)) { fprintf(stderr, "line %d: recorder shape (%d, %d, %d), expected (%d, %d, %d)\n", __LINE__, \
        d_, c_, s_, (int)(d), (int)(cap), (int)(sl)); status = 97; goto done; } } while (0)

ppde_record_config rc_of(int burn_in, int every, int rung, int keep) {
    ppde_record_config r;
    r.burn_in = burn_in; r.every = every; r.rung = rung; r.keep_samples = keep;
    return r;
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
        // default mode on caller-supplied noise: every refusal, then a recorder of every iteration with samples
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        ppde_record_config r = rc_of(0, 1, -1, 1);
        if (refusals) {
            ppde_record_config b;
            EXPECT_INVALID(ppde_chains_set_recorder(nullptr, &r));
            EXPECT_INVALID(ppde_chains_recorder_shape(c0, nullptr, nullptr, nullptr));          // no recorder yet
            b = rc_of(0, 0, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(0, -3, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(-1, 1, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(T, 1, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));          // rows_cap == 0
            b = rc_of(0, T + 1, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(T - 3, 4, -1, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(0, 1, -2, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(0, 1, 0, 1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));           // a rung without tempering
            if (!strstr(ppde_last_error(), "tempering")) { fprintf(stderr, "the refusal does not name tempering: %s\n", ppde_last_error()); status = 95; goto done; }
            b = rc_of(0, 1, -1, 2); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            b = rc_of(0, 1, -1, -1); EXPECT_INVALID(ppde_chains_set_recorder(c0, &b));
            EXPECT_INVALID(ppde_chains_recorder_shape(c0, nullptr, nullptr, nullptr));          // every refusal left the object unchanged
        }
        // the edges of the row schedule: burn_in + every = max_steps is the last recorder with a row
        { ppde_record_config e = rc_of(0, T, -1, 0); TRY(ppde_chains_set_recorder(c0, &e)); EXPECT_SHAPE(c0, 0, 1, n); }
        { ppde_record_config e = rc_of(T - 1, 1, -1, 0); TRY(ppde_chains_set_recorder(c0, &e)); EXPECT_SHAPE(c0, 0, 1, n); }
        { ppde_record_config e = rc_of(T - 7, 7, -1, 1); TRY(ppde_chains_set_recorder(c0, &e)); EXPECT_SHAPE(c0, 0, 1, n); }
        { ppde_record_config e = rc_of(3, 4, -1, 1); TRY(ppde_chains_set_recorder(c0, &e)); EXPECT_SHAPE(c0, 0, (T - 3) / 4, n); }
        TRY(ppde_chains_set_recorder(c0, nullptr));                                             // cleared, then the one the run uses
        TRY(ppde_chains_set_recorder(c0, nullptr));
        TRY(ppde_chains_set_recorder(c0, &r));
        TRY(ppde_chains_set_recorder(c0, &r));                                                  // replaced by itself
        EXPECT_SHAPE(c0, 0, T, n);
        if (refusals) EXPECT_INVALID(ppde_chains_recorder_read(c0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));   // not initialised
        TRY(ppde_chains_init(c0, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_set_recorder(c0, &r));                                    // after init: the graphs hold the pointers
            EXPECT_INVALID(ppde_chains_set_recorder(c0, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(c0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr));   // nothing recorded yet
        }
        EXPECT_SHAPE(c0, 0, T, n);
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        EXPECT_SHAPE(c0, steps, T, n);
        std::vector<uint8_t> si((size_t)steps * n * L);
        std::vector<float> se((size_t)steps * n), sf((size_t)steps * n);
        std::vector<int32_t> sc((size_t)steps * n);
        std::vector<uint64_t> cnt((size_t)L * 20);
        TRY(ppde_chains_recorder_read(c0, 0, steps, si.data(), se.data(), sf.data(), sc.data(), cnt.data()));
        TRY(ppde_chains_recorder_read(c0, 1, 2, si.data(), nullptr, sf.data(), nullptr, nullptr));
        TRY(ppde_chains_recorder_read(c0, steps, 0, si.data(), se.data(), sf.data(), sc.data(), cnt.data()));
        TRY(ppde_chains_recorder_read(c0, 0, steps, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_recorder_read(c0, 0, steps + 1, si.data(), nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(c0, steps, 1, nullptr, se.data(), nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(c0, -1, 1, nullptr, nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(c0, 0, -1, nullptr, nullptr, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
    }
    for (int reuse = 0; reuse <= 1; ++reuse) {
        // device RNG: graphs captured at init (they hold k_record), replayed, then an eager remainder. The first object follows the
        // last rung of a ladder and keeps samples; the second has no ladder and keeps counts only
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = 3; cfg.rng_mode = 1; cfg.reuse_grad = reuse; cfg.random_chain = -1; cfg.nmut_threshold = reuse ? 0 : 4;
        cfg.use_graph = 1; cfg.n_streams = 1; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = reuse ? c2 : c1;
        TRY(ppde_chains_create(&c, m, &cfg));
        const int R = reuse ? 0 : 4, slots = reuse ? n : n / 4;
        ppde_record_config r = rc_of(3, 4, reuse ? -1 : 3, reuse ? 0 : 1);
        if (!reuse) {
            TRY(ppde_chains_set_library(c, lib.data()));
            TRY(ppde_chains_set_reversible(c, 1));
            TRY(ppde_chains_set_tempering(c, R, ladder, 2));
            if (refusals) { ppde_record_config b = rc_of(0, 1, 4, 1); EXPECT_INVALID(ppde_chains_set_recorder(c, &b)); }   // rung >= R
        }
        TRY(ppde_chains_set_recorder(c, &r));
        if (!reuse) {
            if (refusals) {
                EXPECT_INVALID(ppde_chains_set_tempering(c, 0, nullptr, 0));                      // a rung recorder is set: neither cleared ...
                EXPECT_INVALID(ppde_chains_set_tempering(c, 2, ladder, 1));                       // ... nor replaced
                if (!strstr(ppde_last_error(), "recorder")) { fprintf(stderr, "the refusal does not name the recorder: %s\n", ppde_last_error()); status = 95; goto done; }
            }
            TRY(ppde_chains_set_recorder(c, nullptr));                                          // without it the ladder may change again
            TRY(ppde_chains_set_tempering(c, R, ladder, 2));
            TRY(ppde_chains_set_recorder(c, &r));
        }
        EXPECT_SHAPE(c, 0, (2 * T - 3) / 4, slots);
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        EXPECT_SHAPE(c, 0, (2 * T - 3) / 4, slots);                                              // t = 3 = burn_in: nothing yet
        TRY(ppde_chains_run(c, 4, nullptr, nullptr, nullptr, nullptr));
        EXPECT_SHAPE(c, 1, (2 * T - 3) / 4, slots);                                              // t = 7: row 0
        TRY(ppde_chains_run(c, 20, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        if (cap_run != 0 || rep + eag != 30 || rep != 20) { fprintf(stderr, "graph stats: %d captures in run, %lld + %lld steps\n", cap_run, (long long)rep, (long long)eag); status = 96; goto done; }
        const int rows = (30 - 3) / 4;
        EXPECT_SHAPE(c, rows, (2 * T - 3) / 4, slots);
        std::vector<uint64_t> cnt((size_t)L * 20);
        if (reuse) {
            TRY(ppde_chains_recorder_read(c, 0, rows, nullptr, nullptr, nullptr, nullptr, cnt.data()));
            if (refusals) {
                std::vector<uint8_t> si((size_t)rows * slots * L);
                std::vector<float> se((size_t)rows * slots);
                std::vector<int32_t> sc((size_t)rows * slots);
                EXPECT_INVALID(ppde_chains_recorder_read(c, 0, rows, si.data(), nullptr, nullptr, nullptr, cnt.data()));   // counts only
                EXPECT_INVALID(ppde_chains_recorder_read(c, 0, rows, nullptr, se.data(), nullptr, nullptr, nullptr));
                EXPECT_INVALID(ppde_chains_recorder_read(c, 0, rows, nullptr, nullptr, se.data(), nullptr, nullptr));
                EXPECT_INVALID(ppde_chains_recorder_read(c, 0, rows, nullptr, nullptr, nullptr, sc.data(), nullptr));
            }
        } else {
            std::vector<uint8_t> si((size_t)rows * slots * L);
            std::vector<float> se((size_t)rows * slots), sf((size_t)rows * slots);
            std::vector<int32_t> sc((size_t)rows * slots);
            TRY(ppde_chains_recorder_read(c, 0, rows, si.data(), se.data(), sf.data(), sc.data(), cnt.data()));
            TRY(ppde_chains_recorder_read(c, rows - 1, 1, si.data(), se.data(), sf.data(), sc.data(), nullptr));
            std::vector<uint8_t> rh((size_t)31 * n);
            TRY(ppde_chains_tempering_history(c, rh.data()));
        }
    }
    {
        // what the shape of the object refuses: two streams; and a recorder set on an object that is never initialised
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.seed = 5; cfg.chain_offset = 0; cfg.n_streams = 2;
        ppde_record_config r = rc_of(0, 1, -1, 1);
        TRY(ppde_chains_create(&cn, m, &cfg));
        if (refusals) EXPECT_INVALID(ppde_chains_set_recorder(cn, &r));                         // two streams
        TRY(ppde_chains_init(cn, idx.data()));
        if (refusals) {
            EXPECT_INVALID(ppde_chains_recorder_shape(cn, nullptr, nullptr, nullptr));
            EXPECT_INVALID(ppde_chains_recorder_read(cn, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
        }
        TRY(ppde_chains_run(cn, 5, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(cn));
        cfg.n_streams = 1;
        TRY(ppde_chains_create(&ce, m, &cfg));
        TRY(ppde_chains_set_recorder(ce, &r));                                                  // destroyed with its buffers, never run
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
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck recorder ok: %ld fallible runtime calls per walk, %ld injected failures handled\n", walk);
}

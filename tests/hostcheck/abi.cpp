// TEST INFRASTRUCTURE. Drives the whole C ABI of include/ppde_hip.h against the mock runtime (hipmock.cpp) under
// AddressSanitizer + LeakSanitizer: model set-up with all three experts, stateless evaluation, chain objects on both
// RNG modes (eager, graph replay, several streams), peek / collect / trace, argument errors, and — with
// `driver sweep` — the same sequence once per fallible runtime call with that call failing, so every clean-up path
// of the host layer runs. Numbers are meaningless here (kernels do not run); memory errors and leaks are the point.
#include "walk.h"

namespace {
#define EXPECT_FAIL(x) do { if ((x) == PPDE_OK) { fprintf(stderr, "expected an error from %s\n", #x); return 99; } } while (0)

// the full sequence; returns the first non-OK status (after releasing everything it created)
int sequence(int L, int Lp, int win, bool with_tf, bool verbose, int tf_dim = 128, int tf_heads = 4) {
    int status = PPDE_OK;
    ppde_model* m = nullptr;
    ppde_chains *c0 = nullptr, *c1 = nullptr, *c2 = nullptr, *c3 = nullptr;
    const int n = 6, T = 30, N = L * 20;
    std::vector<uint8_t> wt(L);
    for (auto& v : wt) v = rng() % 20;
    std::vector<uint8_t> idx((size_t)n * L);
    for (auto& v : idx) v = rng() % 20;
    // "device" buffers of the caller (the mock's device memory is host memory)
    std::vector<float> e(n), fit(n), grad((size_t)n * N), onehot((size_t)n * N);
    std::vector<uint8_t> back((size_t)n * L);
    TRY(ppde_model_create(&m, 0, L, wt.data()));
    {
        auto J = rnd((size_t)Lp * Lp * 400, 0.05f), h = rnd((size_t)Lp * 20, 0.5f);
        TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));
        TRY(ppde_model_set_potts(m, J.data(), h.data(), Lp, win));                 // replacing an expert frees the old one
        const int C = L, K = 5, F = 2 * L;
        auto cw = many(3, (size_t)C * 20 * K), cb = many(3, C), lw = many(3, (size_t)F * C), lb = many(3, F), dw = many(3, F), db = many(3, 1);
        TRY(ppde_model_set_cnn(m, 3, C, K, F, cw.p.data(), cb.p.data(), lw.p.data(), lb.p.data(), dw.p.data(), db.p.data()));
        TRY(ppde_model_set_cnn(m, 3, C, K, F, cw.p.data(), cb.p.data(), lw.p.data(), lb.p.data(), dw.p.data(), db.p.data()));
        TRY(ppde_model_set_lamda(m, 5.0f));
        float wtH = 0.f;
        TRY(ppde_model_get_wt_hamiltonian(m, &wtH));
    }
    if (with_tf) {
        const int layers = 2, dim = tf_dim, heads = tf_heads, ffn = 256;
        auto emb = rnd((size_t)33 * dim);
        auto qw = many(layers, (size_t)dim * dim), kw = many(layers, (size_t)dim * dim), vw = many(layers, (size_t)dim * dim), ow = many(layers, (size_t)dim * dim);
        auto qb = many(layers, dim), kb = many(layers, dim), vb = many(layers, dim), ob = many(layers, dim);
        auto l1w = many(layers, dim), l1b = many(layers, dim), l2w = many(layers, dim), l2b = many(layers, dim);
        auto f1w = many(layers, (size_t)ffn * dim), f1b = many(layers, ffn), f2w = many(layers, (size_t)dim * ffn), f2b = many(layers, dim);
        auto flw = rnd(dim), flb = rnd(dim), hdw = rnd((size_t)dim * dim), hdb = rnd(dim), hlw = rnd(dim), hlb = rnd(dim), hb = rnd(33);
        ppde_tf_weights w{emb.data(), qw.p.data(), qb.p.data(), kw.p.data(), kb.p.data(), vw.p.data(), vb.p.data(), ow.p.data(), ob.p.data(),
                          l1w.p.data(), l1b.p.data(), l2w.p.data(), l2b.p.data(), f1w.p.data(), f1b.p.data(), f2w.p.data(), f2b.p.data(),
                          flw.data(), flb.data(), hdw.data(), hdb.data(), hlw.data(), hlb.data(), hb.data()};
        TRY(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w));
        TRY(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w));
        float s = 0.f;
        TRY(ppde_model_get_transformer_wt_score(m, &s));
        // a matrix entry that is inf once rounded to fp16, a NaN bias, an inf gain: each refused naming the tensor, before the runtime
        // is touched, and the expert that is there stays (the evaluations below use it)
        float& big = f2w.store[1][7];
        const float keep = big;
        big = 65520.f;
        EXPECT_INVALID(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w), "fc2.weight of layer 1");
        big = -65519.f;                                                              // rounds to -65504: accepted
        TRY(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w));
        big = keep;
        const float keep_b = qb.store[0][3];
        qb.store[0][3] = NAN;
        EXPECT_INVALID(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w), "q_proj.bias of layer 0");
        qb.store[0][3] = keep_b;
        const float keep_g = hlw[0];
        hlw[0] = INFINITY;
        EXPECT_INVALID(ppde_model_set_transformer(m, layers, dim, heads, ffn, &w), "lm_head.layer_norm.weight");
        hlw[0] = keep_g;
        TRY(ppde_model_get_transformer_wt_score(m, &s));
    }
    TRY(ppde_idx_to_onehot(m, idx.data(), n, onehot.data(), nullptr));
    TRY(ppde_onehot_to_idx(m, onehot.data(), n, back.data(), nullptr));
    for (int which = 1; which <= (with_tf ? 15 : 3); ++which) {      // (8..15: PPDE_WHICH_FULL_GRAD on top of 0..7)
        if (!(which & 7)) continue;
        TRY(ppde_energy_grad(m, idx.data(), n, which, e.data(), fit.data(), grad.data(), nullptr));
        TRY(ppde_energy_grad(m, idx.data(), 2, which, e.data(), fit.data(), nullptr, nullptr));   // smaller batch, no gradient
    }
    if (with_tf) {
        std::vector<float> act((size_t)n * L * ((tf_dim + 127) / 128 * 128));
        TRY(ppde_debug_transformer_read(m, 0, 0, act.data(), (int64_t)act.size()));
    }
    {
        // caller-supplied noise, trace on
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.nmut_threshold = 3; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 3; cfg.rng_mode = 0; cfg.trace = 1; cfg.random_chain = 1; cfg.record_after_reset = 1;
        TRY(ppde_chains_create(&c0, m, &cfg));
        TRY(ppde_chains_init(c0, idx.data()));
        const int steps = 4;
        std::vector<int32_t> U((size_t)steps * n, 2), mu(steps, 3);
        for (int t = 0; t < steps; ++t) U[(size_t)t * n] = 3;
        std::vector<float> q((size_t)steps * 3 * n * N, 1.0f), u((size_t)steps * n, 0.5f);
        TRY(ppde_chains_run(c0, steps, U.data(), q.data(), u.data(), mu.data()));
        TRY(ppde_chains_sync(c0));
        std::vector<int32_t> flat((size_t)steps * 3 * n), Ut((size_t)steps * n), dist(n);
        std::vector<uint8_t> acc((size_t)steps * n), pidx((size_t)n * L), pacc(n);
        std::vector<float> la((size_t)steps * n);
        TRY(ppde_chains_trace(c0, flat.data(), acc.data(), la.data(), Ut.data()));
        TRY(ppde_chains_peek(c0, pidx.data(), e.data(), fit.data(), pacc.data(), dist.data()));
        std::vector<uint8_t> bi((size_t)n * L), rt((size_t)(steps + 1) * L);
        std::vector<float> be(n), bf(n), eh((size_t)(steps + 1) * n), fh((size_t)(steps + 1) * n);
        std::vector<int32_t> bs(n);
        TRY(ppde_chains_collect(c0, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), rt.data()));
        if (ppde_chains_steps_done(c0) != steps) { fprintf(stderr, "steps_done\n"); status = 98; goto done; }
    }
    for (int streams = 1; streams <= 2; ++streams) {
        // device RNG: graphs captured at init, replayed; then an eager remainder; timing hooks
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = 2 * T; cfg.pas_length = 3; cfg.min_pos = 0; cfg.max_pos = L - 1;
        cfg.which = with_tf && streams == 1 ? 7 : 3; cfg.rng_mode = 1; cfg.reuse_grad = streams - 1; cfg.random_chain = -1;
        cfg.use_graph = 1; cfg.n_streams = streams; cfg.seed = 11; cfg.chain_offset = 100;
        ppde_chains*& c = streams == 1 ? c1 : c2;
        TRY(ppde_chains_create(&c, m, &cfg));
        TRY(ppde_chains_init(c, idx.data()));
        TRY(ppde_chains_run(c, 27, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_run(c, 3, nullptr, nullptr, nullptr, nullptr));
        TRY(ppde_chains_sync(c));
        int32_t cap = 0, cap_run = 0; int64_t rep = 0, eag = 0;
        TRY(ppde_chains_graph_stats(c, &cap, &cap_run, &rep, &eag));
        float us = 0.f; int launches = 0;
        TRY(ppde_chains_time_potts_kernel(c, 3, &us));
        TRY(ppde_chains_time_experts(c, 2, &us));
        if (ppde_chains_time_potts_in_situ(c, 2, &us, &launches, nullptr) == PPDE_OK) { fprintf(stderr, "in-situ timing accepted an energy with a CNN\n"); status = 97; goto done; }
        std::vector<float> qd((size_t)n * N), ud(n);
        std::vector<int32_t> Ud(n);
        TRY(ppde_chains_philox_dump(c, 0, 0, qd.data(), ud.data(), Ud.data()));
        const int done_steps = ppde_chains_steps_done(c);
        std::vector<uint8_t> bi((size_t)n * L);
        std::vector<float> be(n), bf(n), eh((size_t)(done_steps + 1) * n), fh((size_t)(done_steps + 1) * n);
        std::vector<int32_t> bs(n);
        TRY(ppde_chains_collect(c, bi.data(), be.data(), bf.data(), bs.data(), eh.data(), fh.data(), nullptr));
    }
    {
        // Potts-only energy: the in-situ timing hook (events bound to every dispatch of real iterations)
        ppde_chain_config cfg{};
        cfg.n_chains = n; cfg.max_steps = T; cfg.pas_length = 2; cfg.min_pos = win; cfg.max_pos = win + Lp - 1;
        cfg.which = 1; cfg.rng_mode = 1; cfg.random_chain = -1; cfg.use_graph = 0; cfg.n_streams = 1; cfg.seed = 5;
        TRY(ppde_chains_create(&c3, m, &cfg));
        TRY(ppde_chains_init(c3, idx.data()));
        float us = 0.f, usd = 0.f; int launches = 0;
        TRY(ppde_chains_time_potts_in_situ(c3, 2, &us, &launches, &usd));
        TRY(ppde_chains_time_potts_in_situ(c3, 1, &us, &launches, nullptr));
    }
done:
    if (c3) ppde_chains_destroy(c3);
    if (c0) ppde_chains_destroy(c0);
    if (c1) ppde_chains_destroy(c1);
    if (c2) ppde_chains_destroy(c2);
    if (m) ppde_model_destroy(m);
    return status;
}

int argument_errors() {
    ppde_model* m = nullptr;
    std::vector<uint8_t> wt(40, 3);
    EXPECT_FAIL(ppde_model_create(nullptr, 0, 40, wt.data()));
    EXPECT_FAIL(ppde_model_create(&m, 0, 0, wt.data()));
    EXPECT_FAIL(ppde_model_create(&m, 5, 40, wt.data()));                          // no such device
    if (ppde_model_create(&m, 0, 40, wt.data()) != PPDE_OK) return 97;
    std::vector<float> J((size_t)40 * 40 * 400), h(40 * 20);
    EXPECT_FAIL(ppde_model_set_potts(m, J.data(), h.data(), 41, 0));               // window outside the sequence
    EXPECT_FAIL(ppde_model_set_potts(m, nullptr, h.data(), 40, 0));
    std::vector<uint8_t> idx(40);
    std::vector<float> e(1), fit(1);
    EXPECT_FAIL(ppde_energy_grad(m, idx.data(), 1, 1, e.data(), fit.data(), nullptr, nullptr));   // no Potts expert yet
    EXPECT_FAIL(ppde_energy_grad(m, idx.data(), 1, 0, e.data(), fit.data(), nullptr, nullptr));
    EXPECT_FAIL(ppde_energy_grad(m, idx.data(), 1, 4, e.data(), fit.data(), nullptr, nullptr));   // no transformer expert
    ppde_chain_config cfg{};
    cfg.n_chains = 2; cfg.max_steps = 4; cfg.pas_length = 2; cfg.max_pos = 39; cfg.which = 1;
    ppde_chains* c = nullptr;
    EXPECT_FAIL(ppde_chains_create(&c, m, &cfg));                                    // expert missing
    if (ppde_model_set_potts(m, J.data(), h.data(), 40, 0) != PPDE_OK) return 96;
    cfg.pas_length = 0;
    EXPECT_FAIL(ppde_chains_create(&c, m, &cfg));
    cfg.pas_length = 2; cfg.n_streams = 2;                                           // (ignored with caller-supplied noise: one stream)
    if (ppde_chains_create(&c, m, &cfg) != PPDE_OK) return 95;
    EXPECT_FAIL(ppde_chains_run(c, 1, nullptr, nullptr, nullptr, nullptr));          // not initialised / noise missing
    if (ppde_chains_init(c, std::vector<uint8_t>(80, 1).data()) != PPDE_OK) return 94;
    EXPECT_FAIL(ppde_chains_run(c, 1, nullptr, nullptr, nullptr, nullptr));          // rng_mode 0 without noise
    EXPECT_FAIL(ppde_chains_run(c, 5, nullptr, nullptr, nullptr, nullptr));          // beyond max_steps
    ppde_chains_destroy(c);
    ppde_model_destroy(m);
    return 0;
}

// The shape limits of include/ppde_hip.h that need no kernel result: each refusal is PPDE_ERR_INVALID with a message, happens before
// the object is touched -- across the refused call the runtime sees no kernel launch, no allocation and no copy or fill -- and leaves
// it usable (the mock runs no kernel, so "usable" = the next valid call succeeds and nothing leaks).
// (no clean-up label here: a failed expectation returns its code)
#undef WALK_FAIL
#define WALK_FAIL(code) return (code)
int set_cnn_of(ppde_model* m, int n_nets, int C, int K, int F) {
    const int k = n_nets > 0 ? n_nets : 1, c = C > 0 ? C : 1, kk = K > 0 ? K : 1, f = F > 0 ? F : 1;
    auto cw = many(k, (size_t)c * 20 * kk), cb = many(k, c), lw = many(k, (size_t)f * c), lb = many(k, f), dw = many(k, f), db = many(k, 1);
    return ppde_model_set_cnn(m, n_nets, C, K, F, cw.p.data(), cb.p.data(), lw.p.data(), lb.p.data(), dw.p.data(), db.p.data());
}
int shape_limits() {
    ppde_model* m = nullptr;
    std::vector<uint8_t> wt(4097, 3);
    EXPECT_INVALID(ppde_model_create(&m, 0, 4, wt.data()));
    EXPECT_INVALID(ppde_model_create(&m, 0, 4097, wt.data()));
    if (ppde_model_create(&m, 0, 40, wt.data()) != PPDE_OK) return 97;
    if (set_cnn_of(m, 3, 33, 5, 33) != PPDE_OK) return 96;
    EXPECT_INVALID(set_cnn_of(m, 0, 8, 5, 16));
    EXPECT_INVALID(set_cnn_of(m, 5, 8, 5, 16));
    EXPECT_INVALID(set_cnn_of(m, 3, 8, 0, 16));
    EXPECT_INVALID(set_cnn_of(m, 3, 8, 9, 16));
    EXPECT_INVALID(set_cnn_of(m, 3, 0, 5, 16));
    EXPECT_INVALID(set_cnn_of(m, 3, 8, 5, 0));
    EXPECT_INVALID(set_cnn_of(m, 3, 1024, 5, 64));                                   // wider than the chunk kernels' LDS
    if (!strstr(ppde_last_error(), "channels")) { fprintf(stderr, "the width refusal does not speak of channels: %s\n", ppde_last_error()); return 95; }
    EXPECT_INVALID(set_cnn_of(m, 3, 32, 5, 3201));                                   // more features than the route bitmap holds
    if (!strstr(ppde_last_error(), "features")) { fprintf(stderr, "the F refusal does not speak of features: %s\n", ppde_last_error()); return 95; }
    std::vector<uint8_t> idx(2 * 40, 1);
    std::vector<float> e(2), fit(2), grad((size_t)2 * 40 * 20);
    if (ppde_energy_grad(m, idx.data(), 2, 2, e.data(), fit.data(), grad.data(), nullptr) != PPDE_OK) return 94;   // the expert that was there
    ppde_model_destroy(m); m = nullptr;
    if (ppde_model_create(&m, 0, 7, wt.data()) != PPDE_OK) return 93;
    EXPECT_INVALID(set_cnn_of(m, 3, 8, 8, 16));                                      // K > L
    if (set_cnn_of(m, 3, 8, 7, 16) != PPDE_OK) return 92;                            // K = L: one output row
    ppde_model_destroy(m); m = nullptr;
    // the reference's network shape (C = L, F = 2L) at the last accepted width and one step past it
    if (ppde_model_create(&m, 0, 545, wt.data()) != PPDE_OK) return 91;
    EXPECT_INVALID(set_cnn_of(m, 3, 545, 5, 1090));
    if (!strstr(ppde_last_error(), "channels") || !strstr(ppde_last_error(), "544")) { fprintf(stderr, "L = 545: %s\n", ppde_last_error()); return 90; }
    EXPECT_INVALID(ppde_energy_grad(m, idx.data(), 1, 2, e.data(), fit.data(), nullptr, nullptr));   // no supervised expert was set
    ppde_model_destroy(m); m = nullptr;
    if (ppde_model_create(&m, 0, 544, wt.data()) != PPDE_OK) return 89;
    if (set_cnn_of(m, 3, 544, 5, 1088) != PPDE_OK) { fprintf(stderr, "L = 544: %s\n", ppde_last_error()); return 88; }
    ppde_model_destroy(m); m = nullptr;
    // Potts window of 513 residues: refused before the model is touched (J is never read: a short array will do)
    if (ppde_model_create(&m, 0, 520, wt.data()) != PPDE_OK) return 87;
    std::vector<float> J((size_t)64 * 64 * 400), h(64 * 20);
    EXPECT_INVALID(ppde_model_set_potts(m, J.data(), h.data(), 513, 0));
    std::vector<uint8_t> idx520(520, 2);
    EXPECT_INVALID(ppde_energy_grad(m, idx520.data(), 1, 1, e.data(), fit.data(), nullptr, nullptr));
    float wtH = 0.f;
    EXPECT_INVALID(ppde_model_get_wt_hamiltonian(m, &wtH));
    ppde_chain_config cfg{};
    cfg.n_chains = 2; cfg.max_steps = 4; cfg.pas_length = 2; cfg.max_pos = 519; cfg.which = 1; cfg.rng_mode = 1;
    ppde_chains* c = nullptr;
    EXPECT_INVALID(ppde_chains_create(&c, m, &cfg));
    if (ppde_model_set_potts(m, J.data(), h.data(), 64, 100) != PPDE_OK) return 86;   // a valid window on the same model
    if (ppde_energy_grad(m, idx520.data(), 1, 1, e.data(), fit.data(), nullptr, nullptr) != PPDE_OK) return 85;
    EXPECT_INVALID(ppde_model_set_potts(m, J.data(), h.data(), 513, 0));             // and the refusal leaves THAT expert in place
    if (ppde_energy_grad(m, idx520.data(), 1, 1, e.data(), fit.data(), nullptr, nullptr) != PPDE_OK) return 84;
    EXPECT_INVALID(ppde_chains_create(&c, m, &cfg));                                 // L = 520 > 307
    ppde_model_destroy(m); m = nullptr;
    // chains: L = 308, ppde_pas_length 0 and 65
    if (ppde_model_create(&m, 0, 308, wt.data()) != PPDE_OK) return 83;
    if (ppde_model_set_potts(m, J.data(), h.data(), 64, 100) != PPDE_OK) return 82;
    cfg.max_pos = 307;
    EXPECT_INVALID(ppde_chains_create(&c, m, &cfg));
    ppde_model_destroy(m); m = nullptr;
    if (ppde_model_create(&m, 0, 307, wt.data()) != PPDE_OK) return 81;
    if (ppde_model_set_potts(m, J.data(), h.data(), 64, 100) != PPDE_OK) return 80;
    cfg.max_pos = 306; cfg.pas_length = 0;
    EXPECT_INVALID(ppde_chains_create(&c, m, &cfg));
    cfg.pas_length = 65;
    EXPECT_INVALID(ppde_chains_create(&c, m, &cfg));
    cfg.pas_length = 64;
    if (ppde_chains_create(&c, m, &cfg) != PPDE_OK) { fprintf(stderr, "L = 307, pas 64: %s\n", ppde_last_error()); return 79; }
    std::vector<uint8_t> idx307(2 * 307, 1);
    if (ppde_chains_init(c, idx307.data()) != PPDE_OK || ppde_chains_run(c, 2, nullptr, nullptr, nullptr, nullptr) != PPDE_OK ||
        ppde_chains_sync(c) != PPDE_OK) { fprintf(stderr, "L = 307, pas 64 run: %s\n", ppde_last_error()); return 78; }
    ppde_chains_destroy(c);
    ppde_model_destroy(m);
    return 0;
}

// the shape of a walk for run_walks: this driver keeps its refusals in argument_errors and shape_limits, so both 48-residue walks are
// the plain sequence; the long one (chunked CNN path, ring Potts kernel) runs without the transformer expert
int walk(int L, int Lp, int win, bool verbose, bool) { return sequence(L, Lp, win, L < 100, verbose); }
int more(bool verbose) {
    int rc = sequence(40, 40, 0, true, verbose, 96, 4);                              // head width 24: rows padded 96 -> 128
    if (rc != PPDE_OK) { fprintf(stderr, "head-width-24 run failed\n"); return rc; }
    rc = sequence(40, 40, 0, true, verbose, 256, 4);                                 // head width 64
    if (rc != PPDE_OK) { fprintf(stderr, "head-width-64 run failed\n"); return rc; }
    if ((rc = argument_errors())) { fprintf(stderr, "argument_errors: %d\n", rc); return rc; }
    if ((rc = shape_limits())) fprintf(stderr, "shape_limits: %d\n", rc);
    return rc;
}
}  // namespace

int main(int argc, char** argv) {
    return run_walks(argc, argv, "hostcheck ok: %ld fallible runtime calls per sequence, %ld injected failures handled\n", walk, more);
}

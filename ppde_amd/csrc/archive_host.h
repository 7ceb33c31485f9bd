// The archive on the host: its launch, its fresh start, the setter and the readers. Included by chains.h, where the owner struct
// (Archive) stays with the others: struct ppde_chains holds one of each by value, and all of this needs it complete.
#pragma once

// the archive's kernel for the state after it_base + it_local + 1 completed iterations (archive.h): every chain of the object
static int launch_archive(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Geom& g = c->m->g;
    ArchArgs r{};
    r.it_base = it_base; r.it_local = it_local;
    r.n = c->n; r.K = c->archive.k; r.L = g.L; r.Ls = g.Ls; r.sh = g.sh;
    r.rec = c->rec; r.rec_stride = c->rec_stride; r.cur = c->cur; r.e_hist = c->e_hist; r.f_hist = c->f_hist;
    r.idx = c->archive.idx; r.energy = c->archive.e; r.fitness = c->archive.f; r.step = c->archive.step; r.count = c->archive.count;
    r.hash = c->archive.hash;
    launch_kernel(k_archive, dim3((c->n + ARCH_BLOCK / 64 - 1) / (ARCH_BLOCK / 64)), dim3(ARCH_BLOCK), 0, s, nullptr, r);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// a fresh start: an empty archive, then the initial population as t = 0
static int archive_fresh_start(ppde_chains* c) {
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->archive.count, 0, (size_t)c->n * sizeof(int), s));
    CHK(launch_archive(c, nullptr, -1, s));
    HIPCHK(hipStreamSynchronize(s));
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_archive(ppde_chains* c, const ppde_archive_config* cfg) {
    CHK(set_before_init(c, __func__, "the archive", "the pointers"));
    if (!cfg) return clear_mode(c, c->archive);
    ARGCHK(cfg->k >= 1 && cfg->k <= ARCH_KMAX, "ppde_chains_set_archive: k must be in 1..32");
    ARGCHK(!c->cfg.paper_results, "ppde_chains_set_archive: paper_results is not supported (after a rejection its history row holds the "
                                  "energy of the state that was left while the chain continues from its initial state: a mismatched pair)");
    CHK(one_stream(c, __func__, "one launch archives every chain of the object"));
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    const size_t n = c->n, cells = n * (size_t)cfg->k;
    Archive t;
    t.k = cfg->k;
    CHK(alloc_all(__func__, {{t.idx, cells * (size_t)c->m->g.Ls, true}, {t.e, cells}, {t.f, cells}, {t.step, cells}, {t.hash, cells},
                       {t.count, n, true}}));
    c->archive = std::move(t);
    return PPDE_OK;
}

int ppde_chains_archive_shape(ppde_chains* c, int32_t* k) {
    ARGCHK(c, "null argument");
    ARGCHK(c->archive.on(), "ppde_chains_archive_shape: no archive was set (ppde_chains_set_archive)");
    if (k) *k = c->archive.k;
    return PPDE_OK;
}

int ppde_chains_archive_read(ppde_chains* c, uint8_t* idx, float* energy, float* fitness, int32_t* step, int32_t* count) {
    ARGCHK(c && c->archive.on(), "ppde_chains_archive_read: no archive was set (ppde_chains_set_archive)");
    ARGCHK(c->initialised, "chains not initialised");
    CHK(ppde_chains_sync(c));
    const size_t n = c->n, K = c->archive.k, cells = n * K, L = c->m->g.L;
    std::vector<float> he(cells), hf(cells);
    std::vector<int> hs(cells), hc(n);
    CHK(copy_rows(he.data(), c->archive.e.p, 0, n, K));
    CHK(copy_rows(hf.data(), c->archive.f.p, 0, n, K));
    CHK(copy_rows(hs.data(), c->archive.step.p, 0, n, K));
    CHK(copy_rows(hc.data(), c->archive.count.p, 0, 1, n));
    std::vector<uint8_t> hi;
    if (idx) {
        hi.resize(cells * L);
        CHK(read_state_rows(c, c->archive.idx, n, K, hi.data()));   // [n][K][Ls] -> [n][K][L]
    }
    // each chain's entries by (energy descending, step ascending); the slots beyond count filled
    std::vector<int> order(K);
    for (size_t b = 0; b < n; ++b) {
        const int cnt = std::max(0, std::min(hc[b], (int)K));
        const size_t o = b * K;
        for (int j = 0; j < cnt; ++j) order[j] = j;
        std::sort(order.begin(), order.begin() + cnt, [&](int x, int y) {
            return he[o + x] > he[o + y] || (he[o + x] == he[o + y] && hs[o + x] < hs[o + y]);
        });
        for (size_t j = 0; j < K; ++j) {
            const bool live = (int)j < cnt;
            const size_t src = o + (live ? order[j] : 0);
            if (energy) energy[o + j] = live ? he[src] : -INFINITY;
            if (fitness) fitness[o + j] = live ? hf[src] : 0.f;
            if (step) step[o + j] = live ? hs[src] : -1;
            if (idx) {
                if (live) memcpy(idx + (o + j) * L, hi.data() + src * L, L);
                else memset(idx + (o + j) * L, 255, L);
            }
        }
        if (count) count[b] = cnt;
    }
    return PPDE_OK;
}
}  // extern "C"

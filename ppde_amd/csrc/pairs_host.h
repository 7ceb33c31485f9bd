// The pair counts on the host: their launch, their fresh start, the setter and the readers. Included by chains.h, where the owner
// struct (PairCounts) stays with the others: struct ppde_chains holds one of each by value, and all of this needs it complete.
#pragma once

// the pair counts' kernel for iteration it_base + it_local (pairs.h), on the recorder's schedule and slots; reads cur and slot only
static int launch_pairs(ppde_chains* c, const int* it_base, int it_local, hipStream_t s) {
    const Geom& g = c->m->g;
    const Recorder& rec = c->recorder;
    PairArgs p{};
    p.it_base = it_base; p.it_local = it_local; p.Ls = g.Ls; p.sh = g.sh;
    p.burn_in = rec.cfg.burn_in; p.every = rec.cfg.every; p.rung = rec.cfg.rung; p.n_rungs = c->temper.n_rungs; p.slots = rec.slots;
    p.nt = c->pairs.nt; p.cur = c->cur; p.slot = c->temper.slot; p.sites = c->pairs.sites_dev; p.counts = c->pairs.counts;
    launch_kernel(k_record_pairs, dim3((unsigned)c->pairs.tiles()), dim3(PAIR_BLOCK), 0, s, nullptr, p);
    HIPCHK(hipGetLastError());
    return PPDE_OK;
}

// a fresh start counts from zero
static int pairs_fresh_start(ppde_chains* c) {
    HIPCHK(hipMemset(c->pairs.counts, 0, c->pairs.tiles() * PAIR_TILE * sizeof(unsigned long long)));
    return PPDE_OK;
}

extern "C" {
int ppde_chains_set_pair_counts(ppde_chains* c, const ppde_pair_config* cfg) {
    CHK(set_before_init(c, __func__, "pair counts", "the pointers"));
    if (!cfg) return clear_mode(c, c->pairs);
    ARGCHK(c->recorder.on(), "ppde_chains_set_pair_counts: no recorder was set (pair counts follow its schedule and slots: "
                             "ppde_chains_set_recorder first)");
    const int L = c->m->g.L;
    ARGCHK(cfg->n_sites >= 0 && cfg->n_sites <= L, "ppde_chains_set_pair_counts: n_sites must be in 0..L (0: every residue)");
    ARGCHK(cfg->n_sites == 0 || cfg->sites, "ppde_chains_set_pair_counts: n_sites > 0 needs a site list");
    ARGCHK(cfg->n_sites > 0 || !cfg->sites, "ppde_chains_set_pair_counts: a site list with n_sites = 0 (0 with NULL selects every residue)");
    const int S = cfg->n_sites ? cfg->n_sites : L;
    for (int i = 0; i < cfg->n_sites; ++i) {
        if (cfg->sites[i] < 0 || cfg->sites[i] >= L)
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_pair_counts: sites[" + std::to_string(i) + "] = " + std::to_string(cfg->sites[i]) +
                                          " lies outside the sequence 0.." + std::to_string(L - 1));
        if (i > 0 && cfg->sites[i] <= cfg->sites[i - 1])
            return fail(PPDE_ERR_INVALID, "ppde_chains_set_pair_counts: the sites must be strictly increasing (sites[" + std::to_string(i) +
                                          "] <= sites[" + std::to_string(i - 1) + "])");
    }
    HIPCHK(hipSetDevice(c->device));
    // allocate everything first: a failure leaves the object as it was
    PairCounts t;
    t.nt = (S + PAIR_TS - 1) / PAIR_TS;
    std::vector<int32_t> padded((size_t)t.nt * PAIR_TS, -1);
    for (int i = 0; i < S; ++i) padded[i] = cfg->n_sites ? cfg->sites[i] : i;
    t.sites.assign(padded.begin(), padded.begin() + S);
    CHK(alloc_all(__func__, {{t.sites_dev, padded.size(), padded.data()}, {t.counts, t.tiles() * PAIR_TILE, true}}));
    c->pairs = std::move(t);
    return PPDE_OK;
}

int ppde_chains_pair_counts_shape(ppde_chains* c, int32_t* n_sites, int32_t* sites) {
    ARGCHK(c, "null argument");
    ARGCHK(c->pairs.on(), "ppde_chains_pair_counts_shape: no pair counts were set (ppde_chains_set_pair_counts)");
    if (n_sites) *n_sites = (int32_t)c->pairs.sites.size();
    if (sites) std::copy(c->pairs.sites.begin(), c->pairs.sites.end(), sites);
    return PPDE_OK;
}

int ppde_chains_pair_counts_read(ppde_chains* c, uint64_t* pair_counts) {
    ARGCHK(c && c->initialised, "chains not initialised");
    ARGCHK(c->pairs.on(), "ppde_chains_pair_counts_read: no pair counts were set (ppde_chains_set_pair_counts)");
    CHK(ppde_chains_sync(c));
    if (!pair_counts) return PPDE_OK;
    // the device keeps the upper block triangle, tile by tile (pairs.h): one row of tiles at a time to the host, mirrored here
    const size_t S = c->pairs.sites.size(), W = S * PPDE_A;
    const int nt = c->pairs.nt;
    std::vector<unsigned long long> rowbuf((size_t)nt * PAIR_TILE);
    size_t first = 0;
    for (int ti = 0; ti < nt; ++ti) {
        const size_t tiles = (size_t)(nt - ti);
        CHK(copy_rows(rowbuf.data(), c->pairs.counts.p, first, tiles, (size_t)PAIR_TILE));
        first += tiles;
        for (int tj = ti; tj < nt; ++tj)
            for (int p = 0; p < PAIR_TS; ++p)
                for (int q = 0; q < PAIR_TS; ++q) {
                    const size_t i = (size_t)ti * PAIR_TS + p, j = (size_t)tj * PAIR_TS + q;
                    if (i >= S || j >= S) continue;
                    const unsigned long long* bins = rowbuf.data() + ((size_t)(tj - ti) * PAIR_TS * PAIR_TS + p * PAIR_TS + q) * PAIR_BINS;
                    for (int x = 0; x < PPDE_A; ++x)
                        for (int y = 0; y < PPDE_A; ++y) {
                            const uint64_t v = bins[x * PPDE_A + y];
                            pair_counts[(i * PPDE_A + x) * W + j * PPDE_A + y] = v;
                            if (tj != ti) pair_counts[(j * PPDE_A + y) * W + i * PPDE_A + x] = v;
                        }
                }
    }
    return PPDE_OK;
}
}  // extern "C"

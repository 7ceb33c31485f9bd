// The plan's kernel, included twice by anneal.h: as k_select_plan (ANNEAL_PLAN_ADAPTIVE 0, the fixed schedule) and as
// k_select_plan_adaptive (ANNEAL_PLAN_ADAPTIVE 1, which also takes AnnealStepArgs x). Two kernels from one text, not two
// instantiations of a template: a template's static LDS arrays get another linkage and the compiler then allocates the fixed
// kernel's registers differently; this way the fixed kernel's instructions stay exactly what they were before the adaptive form.
#if ANNEAL_PLAN_ADAPTIVE
__global__ __launch_bounds__(ANNEAL_BLOCK) void k_select_plan_adaptive(AnnealArgs a, AnnealStepArgs x) {
#else
__global__ __launch_bounds__(ANNEAL_BLOCK) void k_select_plan(AnnealArgs a) {
    const AnnealStepArgs x{};                        // (named in the discarded branches only)
#endif
    constexpr bool ADAPTIVE = ANNEAL_PLAN_ADAPTIVE;
    int it;
    const int s = anneal_stage(a, it);
    if (s < 0) return;
    __shared__ double C[ANNEAL_DMAX];                // inclusive prefix sums of the weights
    __shared__ int cnt[ANNEAL_DMAX];                 // offspring counts
    __shared__ int lst[ANNEAL_DMAX];                 // the surplus list
    __shared__ double xd[2 * ANNEAL_NW];
    __shared__ float xf[ANNEAL_NW];
    __shared__ int xi[ANNEAL_NW];
    const int D = a.D, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int first = blockIdx.x * D;                // local index of the deme's first chain
    const int i0 = tid * ANNEAL_CPT;
    const float* erow = a.e_hist + (size_t)(it + 1) * a.n + first;
    double db = ADAPTIVE ? 0.0 : (double)a.sched[s + 1] - (double)a.sched[s];
    // the adaptive form: the deme's beta (written at the end of this launch, behind barriers, by this workgroup alone) and its choice
    float b_cur = 0.f, b_step = 0.f;
    if constexpr (ADAPTIVE) b_cur = b_step = a.beta[first];

    float e[ANNEAL_CPT];
    bool fin[ANNEAL_CPT];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        const int i = i0 + r;
        e[r] = i < D ? erow[i] : -INFINITY;
        fin[r] = i < D && fabsf(e[r]) < INFINITY;    // (false for NaN and both infinities)
        if (fin[r]) mx = fmaxf(mx, e[r]);
        cnt[i] = 0;
    }
    mx = wave_max(mx);
    if (lane == 0) xf[wave] = mx;
    __syncthreads();
    float emax_f = xf[0];
#pragma unroll
    for (int w = 1; w < ANNEAL_NW; ++w) emax_f = fmaxf(emax_f, xf[w]);
    const bool any = emax_f > -INFINITY;             // a finite energy in the deme
    const double emax = (double)emax_f;

    if constexpr (ADAPTIVE) {
        __shared__ double xa[4 * ANNEAL_NW];
        __shared__ int xn[ANNEAL_NW];
        const double b0 = (double)b_cur, dmax = (double)x.beta_end - b0;
        if (any && dmax > 0.0) {                     // (uniform: emax_f and beta[first] are the same in every thread)
            double xe[ANNEAL_CPT];
            int nf = 0;
#pragma unroll
            for (int r = 0; r < ANNEAL_CPT; ++r) { xe[r] = fin[r] ? (double)e[r] - emax : 0.0; nf += fin[r] ? 1 : 0; }
            nf = wave_scan_incl_i(nf);
            if (lane == 63) xn[wave] = nf;
            __syncthreads();
            int F = 0;
#pragma unroll
            for (int k = 0; k < ANNEAL_NW; ++k) F += xn[k];
            const double target = (double)x.rho * (double)F;
            int turn = 0;
            double tot, sq, d = dmax;
            anneal_ess_sums(dmax, xe, fin, xa, turn, tot, sq);
            if (!(tot * tot / sq >= target)) {
                double lo = 0.0, hi = dmax;
#pragma nounroll
                for (int k = 0; k < 48; ++k) {
                    const double mid = 0.5 * (lo + hi);
                    anneal_ess_sums(mid, xe, fin, xa, turn, tot, sq);
                    if (tot * tot / sq >= target) lo = mid; else hi = mid;
                }
                d = fmax(lo, (double)x.min_step);
            }
            const float b_try = (float)(b0 + d);     // round to nearest
            b_step = (d >= dmax || b_try >= x.beta_end) ? x.beta_end : b_try;
            db = (double)b_step - b0;
        }
    }

    double w[ANNEAL_CPT], tot = 0.0, sq = 0.0;
    int last = -1;
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        w[r] = fin[r] ? exp(db * ((double)e[r] - emax)) : 0.0;
        tot += w[r];
        sq += w[r] * w[r];
        if (w[r] > 0.0) last = i0 + r;
    }
    const double incl = wave_scan_incl_d(tot);
    const double sq_w = wave_sum_d(sq);
    last = (int)wave_max((float)last);               // (indices below 2^24: exact in fp32)
    if (lane == 63) xd[wave] = incl;
    if (lane == 0) { xd[ANNEAL_NW + wave] = sq_w; xi[wave] = last; }
    __syncthreads();
    double off = 0.0, sumsq = 0.0;
    int last_pos = -1;
#pragma unroll
    for (int k = 0; k < ANNEAL_NW; ++k) {
        off += k < wave ? xd[k] : 0.0;
        sumsq += xd[ANNEAL_NW + k];
        last_pos = max(last_pos, xi[k]);
    }
    {
        double c = off + incl - tot;                 // exclusive prefix of this thread
#pragma unroll
        for (int r = 0; r < ANNEAL_CPT; ++r) { c += w[r]; C[i0 + r] = c; }
    }
    __syncthreads();
    const double W = C[D - 1];
    const bool select = any && W > 0.0;

    if (select) {
        const U4 rnd = philox4x32_10(U4{a.key.chain_lo + (uint32_t)first, (uint32_t)it, ANNEAL_STREAM, 0u}, a.key.k0, a.key.k1);
        const double u = (double)unif_from_bits(rnd.x), step = W / (double)D;
#pragma unroll
        for (int r = 0; r < ANNEAL_CPT; ++r) {
            const int j = i0 + r;
            if (j >= D) continue;
            const double tau = ((double)j + u) * step;
            int lo = 0, hi = D;                      // first i with C_i > tau = #{i : C_i <= tau}
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (C[mid] <= tau) lo = mid + 1; else hi = mid;
            }
            atomicAdd(&cnt[min(lo, last_pos)], 1);
        }
    }
    __syncthreads();
    int nd = 0, ns = 0, c_i[ANNEAL_CPT];
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        c_i[r] = (select && i0 + r < D) ? cnt[i0 + r] : 1;
        nd += c_i[r] == 0 ? 1 : 0;
        ns += c_i[r] > 1 ? c_i[r] - 1 : 0;
    }
    int total_dead, total_surplus;
    int dx = anneal_scan_excl_i(nd, xi, total_dead);
    int sx = anneal_scan_excl_i(ns, xi, total_surplus);
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r)
        for (int k = 1; k < c_i[r]; ++k) lst[min(sx++, ANNEAL_DMAX - 1)] = i0 + r;     // (sum (n_i - 1)+ = dead slots <= D - 1)
    __syncthreads();
    const size_t row = (size_t)s * a.n + first;
    const float b_next = ADAPTIVE ? b_step : a.sched[s + 1];
#pragma unroll
    for (int r = 0; r < ANNEAL_CPT; ++r) {
        const int i = i0 + r;
        if (i >= D) continue;
        int p = i;
        if (c_i[r] == 0) { p = lst[min(dx, ANNEAL_DMAX - 1)]; ++dx; }
        a.parent[row + i] = first + p;
        a.pre_energy[row + i] = e[r];
        a.beta[first + i] = b_next;
    }
    if (tid == 0) {
        const size_t cell = (size_t)s * (a.n / D) + blockIdx.x;
        a.log_mean_w[cell] = select ? log(W / (double)D) + db * emax : -INFINITY;
        a.ess[cell] = select ? W * W / sumsq : 0.0;
        if constexpr (ADAPTIVE) {
            x.beta_pair[cell] = b_cur;
            x.beta_pair[(size_t)x.cap * (a.n / D) + cell] = b_next;
        }
    }
}

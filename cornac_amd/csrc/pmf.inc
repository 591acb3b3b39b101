// PMF: the reference's sequential per-rating RMSProp factorisation, in float64 — included at the end of mf.hip, on the MF handle.
//
// Replaces pmf_linear / pmf_non_linear (cornac/models/pmf/cython/pmf.pyx:55-111, :115-173): per epoch, for every rating in
// stored order, on ONE thread always (no prange, no racy mode):
//     s  = sum_f U[u,f] V[i,f]                               (index order, from 0.0)
//     e  = val - s                 w = e                      linear
//     sg = sigmoid(s), e = val - sg, w = e sg (1. - sg)       non-linear (float sigmoid(float): s rounded to float, 1 above
//                                                             6, 0 below -6, else 1/(1+expf(-z)) in double rounded to float)
//     user row:  g = w V - reg U;  cache = gamma cache + (1 - gamma) (g g);  U += lr (g / (sqrt(cache) + 1e-8))
//     item row:  the same with the ALREADY UPDATED U against the not yet updated V
//     loss[epoch] += e e + reg (|U_new|^2 + |V_new|^2)
// Types as in the C that Cython generates: tables, caches, s, e, w, sg, eps are double; lambda_reg, learning_rate and gamma
// are C floats promoted in every product; (1 - gamma) is evaluated in float; rat[r] is a float promoted to double.  Every
// operation is a correctly rounded IEEE double + - * / sqrt in that order, contraction off: the factors are bit-identical
// to the sequential loop's (the sigmoid's expf is evaluated the way the host's libm does it: pmf_expf).
//
//   pmf_det_level_kernel  one launch per level of the row-conflict DAG (mf_build_schedule): k > 256, nnz < 4096, and after
//                         a refused cooperative launch
//   pmf_det_chain_kernel  the dataflow driver of chain.h (one persistent launch, owned rows in stored order by one wave,
//                         shared rows handed over by version counters: the protocol is explained there) on MF's plan, with
//                         this per-rating body and four float64 tables: the shared side's parameter row AND its cache row
//                         travel with system-scope 8-byte loads and stores, the owned side's with plain ones.
//
// Several ratings per wave pass (G < 64).  PMF's default is k = 5: one rating per wave would leave 59 lanes idle on a
// latency-bound kernel.  The ratings one poll finds ready are mutually independent (chain.h), so for k <= 32 the ready
// set runs in lane groups of G = pow2 >= k (8, 16, 32 lanes: 8, 4, 2 ratings per pass).

namespace chip {

struct PmfHyper {
    double lr, reg, gamma, one_minus_gamma;  // the reference's float arguments (and its float 1 - gamma), promoted
};

// expf(x), |x| <= 6, the way the host's libm evaluates it (glibc >= 2.27, the scheme of Arm's optimized routines): all in
// double — x 32 / ln2 = k + r with k integer and |r| <= 1/2 (the add-and-subtract of 1.5 x 2^52 rounds to nearest even),
// exp(x) = 2^(k/32) 2^(r/32) ~= s (C0 r^3 + C1 r^2 + C2 r + 1) with s from a 32-entry table of 2^(i/32) whose exponent
// field takes k / 32 — and ONE rounding to float at the end.  Unfused, operation for operation, so the float is the
// host's bit for bit (a libm built with fused multiply-adds differs in the last bit of the DOUBLE: the float then differs
// only where that double lies within 2^-53 of a rounding boundary, about once in 2^29 calls).  The table entries are
// bits(2^(i/32) correctly rounded) - (i << 47).
__constant__ unsigned long long kPmfExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull,
    0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull,
    0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull,
    0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull,
    0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
    0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

__device__ __forceinline__ float pmf_expf(float x) {
    constexpr double kInvLn2N = 0x1.71547652b82fep+0 * 32, kShift = 0x1.8p+52;
    constexpr double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32, C2 = 0x1.62e42ff0c52d6p-1 / 32;
    const double z = kInvLn2N * (double)x;
    double kd = z + kShift;
    const unsigned long long ki = __builtin_bit_cast(unsigned long long, kd);
    kd = kd - kShift;
    const double r = z - kd;
    const double s = __builtin_bit_cast(double, kPmfExp2fTab[ki & 31ull] + (ki << 47));
    const double p = C0 * r + C1;
    const double r2 = r * r;
    double y = C2 * r + 1.0;
    y = p * r2 + y;
    y = y * s;
    return (float)y;
}

// cdef float sigmoid(float z), pmf.pyx:27-37.  The reference builds this extension as C++ (setup.py:161-165), where
// `exp(-z)` with a float z is the FLOAT overload: expf(-z), then 1.0 / (1.0 + that) in double, rounded to float.
__device__ __forceinline__ float pmf_sigmoid(float z) {
    if (z > 6.0f) return 1.0f;
    if (z < -6.0f) return 0.0f;
    return (float)(1.0 / (1.0 + (double)pmf_expf(-z)));
}

// e and the weight of the two row gradients (pmf.pyx:84 | :144-146)
template <int VARIANT>
__device__ __forceinline__ void pmf_errors(double val, double s, double &e, double &w) {
    if (VARIANT == CORNAC_HIP_PMF_NON_LINEAR) {
        const double sg = (double)pmf_sigmoid((float)s);
        e = val - sg;
        w = e * sg * (1. - sg);
    } else {
        e = val - s;
        w = e;
    }
}

// one factor of one row (pmf.pyx:88-90): p and its RMSProp cache c against the other row's factor
__device__ __forceinline__ void pmf_row_step(double w, double other, double &p, double &c, const PmfHyper &hy) {
    const double g = w * other - hy.reg * p;
    c = hy.gamma * c + hy.one_minus_gamma * (g * g);
    p = p + hy.lr * (g / (sqrt(c) + 1e-8));
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const unsigned long long x = __builtin_bit_cast(unsigned long long, v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)x, l);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(x >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// acc = ((acc + p[0]) + p[1]) + ... + p[lim-1] over the lanes of a G-lane group, in lane order (ordered_lane_sum_t; a whole
// wave reads every term with v_readlane)
template <int G>
__device__ __forceinline__ double pmf_ordered_sum(double acc, double p, int lim) {
    if (G == kWave) {
#pragma unroll
        for (int l = 0; l < kWave; ++l)
            if (l < lim) acc = acc + readlane_f64(p, l);
        return acc;
    }
    return ordered_lane_sum_t<G>(acc, p, lim);
}

template <int G, int VARIANT>
__global__ __launch_bounds__(kBlock) void pmf_det_level_kernel(const int32_t *__restrict__ ou, const int32_t *__restrict__ oi,
                                                               const float *__restrict__ orat, int64_t off, int cnt, double *U,
                                                               double *V, double *CU, double *CV, int k, const PmfHyper hy,
                                                               double *__restrict__ loss_acc) {
    const int gid = (blockIdx.x * kBlock + threadIdx.x) / G;
    const int lg = threadIdx.x & (G - 1);
    const bool active = gid < cnt;
    const int64_t t = off + (active ? gid : cnt - 1);
    const int32_t u = ou[t], i = oi[t];
    const double val = (double)orat[t];
    double *pu = U + (size_t)u * k, *pi = V + (size_t)i * k, *pcu = CU + (size_t)u * k, *pcv = CV + (size_t)i * k;
    double s = 0.0;
    for (int base = 0; base < k; base += G) {
        const int f = base + lg;
        double p = 0.0;
        if (f < k) p = pu[f] * pi[f];
        s = pmf_ordered_sum<G>(s, p, min(G, k - base));
    }
    double e, w;
    pmf_errors<VARIANT>(val, s, e, w);
    double nrm = 0.0;
    if (active) {
        for (int f = lg; f < k; f += G) {
            const double v_old = pi[f];
            double un = pu[f], cun = pcu[f], vn = v_old, cvn = pcv[f];
            pmf_row_step(w, v_old, un, cun, hy);
            pmf_row_step(w, un, vn, cvn, hy);
            pu[f] = un;
            pcu[f] = cun;
            pi[f] = vn;
            pcv[f] = cvn;
            nrm += un * un + vn * vn;
        }
    }
    // loss: partial sums in another order than the reference's (compared with a tolerance)
    const double l = wave_sum_f64(active ? (lg == 0 ? e * e : 0.0) + hy.reg * nrm : 0.0);
    if (lane_id() == 0 && l != 0.0) atomicAdd(loss_acc, l);
}

struct PmfChainArgs {
    ChainArgs c;                    // the plan of mf_build_chain
    double *U, *V, *CU, *CV;
    double *loss_acc;
    int k;
    PmfHyper hy;
};

// k <= G R; G < 64 (R == 1): 64 / G ready ratings per pass, one per lane group
template <int G, int R, bool OWN_USER, int VARIANT>
__global__ __launch_bounds__(kBlock) void pmf_det_chain_kernel(const PmfChainArgs a) {
    static_assert(G == kWave || R == 1, "lane groups hold a whole row");
    double err2 = 0.0, nrm = 0.0;
    chain_run<G>(a.c, [&](const ChainPass p) {
        const int32_t u = OWN_USER ? p.oid : p.sid, i = OWN_USER ? p.sid : p.oid;
        double *pu = a.U + (size_t)u * a.k, *pi = a.V + (size_t)i * a.k;
        double *pcu = a.CU + (size_t)u * a.k, *pcv = a.CV + (size_t)i * a.k;
        double uf[R], vf[R], cu[R], cv[R];
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int f = p.lg + G * c;
            const bool in = p.act && f < a.k;
            uf[c] = in ? (OWN_USER ? pu[f] : load_f64_sys(pu + f)) : 0.0;
            vf[c] = in ? (OWN_USER ? load_f64_sys(pi + f) : pi[f]) : 0.0;
            cu[c] = in ? (OWN_USER ? pcu[f] : load_f64_sys(pcu + f)) : 0.0;
            cv[c] = in ? (OWN_USER ? load_f64_sys(pcv + f) : pcv[f]) : 0.0;
        }
        // ---- the reference's expression tree (pmf_det_level_kernel) ----
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (G * c < a.k) dot = pmf_ordered_sum<G>(dot, uf[c] * vf[c], min(G, a.k - G * c));
        }
        double e, wt;
        pmf_errors<VARIANT>((double)p.r, dot, e, wt);
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int f = p.lg + G * c;
            if (p.act && f < a.k) {
                double un = uf[c], cun = cu[c], vn = vf[c], cvn = cv[c];
                pmf_row_step(wt, vf[c], un, cun, a.hy);
                pmf_row_step(wt, un, vn, cvn, a.hy);
                if (OWN_USER) {
                    pu[f] = un;
                    pcu[f] = cun;
                    store_f64_sys(pi + f, vn);
                    store_f64_sys(pcv + f, cvn);
                } else {
                    store_f64_sys(pu + f, un);
                    store_f64_sys(pcu + f, cun);
                    pi[f] = vn;
                    pcv[f] = cvn;
                }
                nrm += un * un + vn * vn;
            }
        }
        if (p.act && p.lg == 0) err2 += e * e;
    });
    const double l = wave_sum_f64(err2 + a.hy.reg * nrm);
    if (lane_id() == 0 && l != 0.0) atomicAdd(a.loss_acc, l);
}

}  // namespace chip

// ---- host: kernel choice, schedule, epochs -----------------------------------------------------------------------------
typedef void (*PmfChainKernel)(const PmfChainArgs);

// lanes of a rating's group in the dataflow kernel: pow2 >= k up to 32 when grouped, else the whole wave
static int pmf_chain_group(int k, bool grouped) {
    if (!grouped || k > 32) return kWave;
    return k <= 8 ? 8 : k <= 16 ? 16 : 32;
}

template <bool OWN_USER, int VARIANT>
static PmfChainKernel pick_pmf_chain_kernel_t(int k, int G) {
    if (G == 8) return pmf_det_chain_kernel<8, 1, OWN_USER, VARIANT>;
    if (G == 16) return pmf_det_chain_kernel<16, 1, OWN_USER, VARIANT>;
    if (G == 32) return pmf_det_chain_kernel<32, 1, OWN_USER, VARIANT>;
    if (k <= 64) return pmf_det_chain_kernel<64, 1, OWN_USER, VARIANT>;
    if (k <= 128) return pmf_det_chain_kernel<64, 2, OWN_USER, VARIANT>;
    if (k <= 192) return pmf_det_chain_kernel<64, 3, OWN_USER, VARIANT>;
    return pmf_det_chain_kernel<64, 4, OWN_USER, VARIANT>;
}

static PmfChainKernel pick_pmf_chain_kernel(int k, int G, bool own_user, int variant) {
    if (variant == CORNAC_HIP_PMF_NON_LINEAR)
        return own_user ? pick_pmf_chain_kernel_t<true, CORNAC_HIP_PMF_NON_LINEAR>(k, G)
                        : pick_pmf_chain_kernel_t<false, CORNAC_HIP_PMF_NON_LINEAR>(k, G);
    return own_user ? pick_pmf_chain_kernel_t<true, CORNAC_HIP_PMF_LINEAR>(k, G)
                    : pick_pmf_chain_kernel_t<false, CORNAC_HIP_PMF_LINEAR>(k, G);
}

// workgroups per CU the dataflow plan may count on for this handle's PMF kernels: the smallest answer of the occupancy
// query over the forms a later call may pick (either owned side, either variant); mf_build_chain halves it
static int pmf_chain_per_cu(cornac_hip_mf_t h, int G) {
    int per_cu = 8;
    for (int own = 0; own < 2; ++own)
        for (int variant = 0; variant < 2; ++variant) {
            int q = 0;
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, pick_pmf_chain_kernel(h->k, G, own != 0, variant), kBlock, 0));
            per_cu = std::min(per_cu, q);
        }
    return per_cu;
}

template <int G>
static void launch_pmf_level(cornac_hip_mf_t h, int64_t off, int cnt, const PmfHyper &hy, int variant, double *loss_slot) {
    const int groups_per_block = kBlock / G;
    const int grid = (cnt + groups_per_block - 1) / groups_per_block;
    if (variant == CORNAC_HIP_PMF_NON_LINEAR)
        hipLaunchKernelGGL((pmf_det_level_kernel<G, CORNAC_HIP_PMF_NON_LINEAR>), dim3(grid), dim3(kBlock), 0, h->stream, h->ou.p,
                           h->oi.p, h->orat.p, off, cnt, h->pmf_U.p, h->pmf_V.p, h->pmf_cu.p, h->pmf_cv.p, h->k, hy, loss_slot);
    else
        hipLaunchKernelGGL((pmf_det_level_kernel<G, CORNAC_HIP_PMF_LINEAR>), dim3(grid), dim3(kBlock), 0, h->stream, h->ou.p,
                           h->oi.p, h->orat.p, off, cnt, h->pmf_U.p, h->pmf_V.p, h->pmf_cu.p, h->pmf_cv.p, h->k, hy, loss_slot);
}

static void pmf_epoch_levels(cornac_hip_mf_t h, const PmfHyper &hy, int variant, double *loss_slot) {
    mf_build_schedule(h);
    const int G = h->k <= 8 ? 8 : h->k <= 16 ? 16 : h->k <= 32 ? 32 : 64;
    const std::vector<int64_t> &lp = h->sched.level_ptr;
    for (size_t l = 1; l + 1 < lp.size(); ++l) {
        const int64_t off = lp[l];
        const int cnt = (int)(lp[l + 1] - lp[l]);
        if (cnt <= 0) continue;
        switch (G) {
            case 8: launch_pmf_level<8>(h, off, cnt, hy, variant, loss_slot); break;
            case 16: launch_pmf_level<16>(h, off, cnt, hy, variant, loss_slot); break;
            case 32: launch_pmf_level<32>(h, off, cnt, hy, variant, loss_slot); break;
            default: launch_pmf_level<64>(h, off, cnt, hy, variant, loss_slot); break;
        }
    }
    h->pmf_form = 2;
    h->pmf_group = kWave / G;
    HIP_CHECK(hipGetLastError());
}

// as mf_epoch_chain: false when the runtime refuses the cooperative launch (nothing has run)
static bool pmf_epoch_chain(cornac_hip_mf_t h, int G, const PmfHyper &hy, int variant, double *loss_slot) {
    PmfChainArgs a;
    a.c = chain_args(h->chain, h->c_sid.p, h->c_seq.p, h->c_r.p);
    a.U = h->pmf_U.p; a.V = h->pmf_V.p; a.CU = h->pmf_cu.p; a.CV = h->pmf_cv.p; a.loss_acc = loss_slot;
    a.k = h->k; a.hy = hy;
    return chain_launch(h->stream, h->chain, pick_pmf_chain_kernel(h->k, G, h->chain_own_user, variant), &a, "PMF dataflow kernel");
}

extern "C" {

int cornac_hip_mf_pmf_set_factors(cornac_hip_mf_t h, const double *U, const double *V) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(U && V, "U and V are required");
        const size_t nu = (size_t)h->n_users * h->k, ni = (size_t)h->n_items * h->k;
        h->pmf_U.ensure(nu); h->pmf_cu.ensure(nu);
        h->pmf_V.ensure(ni); h->pmf_cv.ensure(ni);
        h->pmf_U.upload(U, nu, h->stream);
        h->pmf_V.upload(V, ni, h->stream);
        HIP_CHECK(hipMemsetAsync(h->pmf_cu.p, 0, nu * sizeof(double), h->stream));
        HIP_CHECK(hipMemsetAsync(h->pmf_cv.p, 0, ni * sizeof(double), h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->pmf_set = true;
    });
}

int cornac_hip_mf_pmf_get_factors(cornac_hip_mf_t h, double *U, double *V) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(h->pmf_set, "cornac_hip_mf_pmf_set_factors has not been called on this handle");
        if (U) h->pmf_U.download(U, (size_t)h->n_users * h->k, h->stream);
        if (V) h->pmf_V.download(V, (size_t)h->n_items * h->k, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_mf_pmf_fit(cornac_hip_mf_t h, int n_epochs, float lr, float reg, float gamma, int variant, double *loss_per_epoch) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        REQUIRE(h->pmf_set, "cornac_hip_mf_pmf_fit before cornac_hip_mf_pmf_set_factors");
        REQUIRE(variant == CORNAC_HIP_PMF_LINEAR || variant == CORNAC_HIP_PMF_NON_LINEAR, "unknown PMF variant %d", variant);
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        mf_check(h);
        const float one_minus_gamma = 1.0f - gamma;   // `(1 - gamma)` with a C float gamma: float arithmetic (pmf.pyx:89)
        const PmfHyper hy = {(double)lr, (double)reg, (double)gamma, (double)one_minus_gamma};
        h->pmf_loss.ensure((size_t)std::max(n_epochs, 1));
        HIP_CHECK(hipMemsetAsync(h->pmf_loss.p, 0, h->pmf_loss.n * sizeof(double), h->stream));
        const int G = pmf_chain_group(h->k, !prof_env_set("CORNAC_HIP_PMF_ONE_PER_WAVE"));
        bool chain = mf_uses_chain(h) && !h->pmf_chain_refused && !prof_env_set("CORNAC_HIP_MF_LEVELS");
        if (chain) {
            // the plan is sized to half of what the occupancy query admits for THIS kernel (more registers than MF's); a
            // plan an MF fit of the handle has already sized beyond that is not used
            const int per_cu = pmf_chain_per_cu(h, G);
            mf_build_chain(h, per_cu);
            chain = h->chain.grid <= device_info(h->device).cus * std::max(1, std::min(per_cu, 8) / 2);
        }
        for (int e = 0; e < n_epochs; ++e) {
            if (chain && pmf_epoch_chain(h, G, hy, variant, h->pmf_loss.p + e)) {
                h->pmf_form = 1;
                h->pmf_group = kWave / G;
                continue;
            }
            if (chain) {   // the dataflow launch was refused before anything ran: the level schedule from now on
                chain = false;
                h->pmf_chain_refused = true;
            }
            pmf_epoch_levels(h, hy, variant, h->pmf_loss.p + e);
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (loss_per_epoch && n_epochs > 0)
            HIP_CHECK(hipMemcpy(loss_per_epoch, h->pmf_loss.p, sizeof(double) * (size_t)n_epochs, hipMemcpyDeviceToHost));
    });
}

int cornac_hip_mf_pmf_form(cornac_hip_mf_t h, int *form, int *group) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        if (form) *form = h->pmf_form;
        if (group) *group = h->pmf_group;
    });
}
}

// HPF: Poisson factorisation's variational updates in float64 — included at the end of mf.hip, on the MF handle.
//
// Replaces hpf_cpp / pf_cpp (cornac/models/hpf/cpp/cpp_hpf.cpp:208-275 / :139-203) as hpf.pyx:100-164 / :35-97 call them.
// Four tables G_s, G_r [n_users, k], L_s, L_r [n_items, k] and two vectors K_r [n_users], T_r [n_items].  One iteration:
//   1. Lt = exp(digamma(G_s) - log G_r), Lb = exp(digamma(L_s) - log L_r)            (E_SpMat_logGamma, :102-123, + exp)
//   2. G_s[u,f] = prior + sum over the ratings of u of Lt[u,f] Lb[i,f] x / dk,  dk = eps + sum_f Lt[u,f] Lb[i,f]   (:41-61)
//   3. G_r[u,f] = k_s / K_r[u] + sum_j L_s[j,f] / L_r[j,f]   — the L of the iteration before                        (:22-37)
//   4. hierarchical: K_r[u] = 0.3 + sum_f G_s[u,f] / G_r[u,f]                                                         (:7-19)
//   5. L_s[i,f] = prior + the sums of step 2 by item, from the Lt and Lb of step 1                                   (:65-84)
//   6. L_r[i,f] = t_s / T_r[i] + sum_u G_s[u,f] / G_r[u,f]   — the G of steps 2 and 3
//   7. hierarchical: T_r likewise from L
// eps = 2^-52, prior = 0.3, k_s = t_s = 0.3 (1 + k) hierarchical / 0.3 otherwise.  The tables must be strictly positive and
// finite: the reference's detour through pruned sparse matrices (:111-118) is the dense formula then.  Its treatment of
// zeros is not reproduced.
//
//   hpf_elog_kernel     step 1 over (n_users + n_items) k elements; the digamma is the recurrence psi(x) = psi(x + 1) - 1/x up
//                       to x >= 10, then the asymptotic series in 1/x^2.  A tiny shape gives psi = -1/x, exp underflows: Lt = 0.
//   hpf_sum_kernel      steps 2 and 5: nmf_sum_kernel's walk in double.  A lane group of G = pow2 >= k lanes (8..64; k <= 256:
//                       up to four slices of 64) owns a segment of one row of NMF's split plan and walks it in ascending
//                       position, its k sums in registers; per rating it gathers the other side's row, sums dk across the
//                       group with a butterfly and adds P x / dk.  Whole rows start from the prior; the pieces of a row longer
//                       than kNmfSplit start from zero and hpf_combine_kernel adds them onto the prior in ascending order.
//                       One owner per accumulator row, no float atomics: the same bits run to run.  The item side walks
//                       NMF's CSC permutation and computes dk again (the same products, the same butterfly: the same bits
//                       as the user side's) — or, DK = 1 / 2, the user side stores dk per rating and the item side reads it.
//   hpf_colsum_kernel   the column sums of steps 3 and 6: a fixed split of the rows over workgroups, a serial sum per thread,
//                       a tree over LDS, then the same kernel once more over the workgroups' partials.  No atomics.
//   hpf_rate_kernel     steps 3 + 4 / 6 + 7: one lane group per row writes the rate, then sums shape / rate over the row.
// There is one mode: the reference runs on one thread always and its own summation order cannot be held bit for bit (three
// library functions differ), so every sum here takes a fixed order of its own.

namespace chip {

constexpr int kHpfMaxK = 256;
constexpr double kHpfPrior = 0.3;   // a_ (and b_ / c_ of the item side): cpp_hpf.cpp:149-151, :218-220

// psi(x), x > 0
__device__ __forceinline__ double hpf_digamma(double x) {
    double r = 0.0;
    for (int n = 0; n < 10 && x < 10.0; ++n) {   // at most ten steps for any x > 0
        r = r - 1.0 / x;
        x = x + 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    // sum B_2n / (2n x^2n), n = 1..8 (the next term is below 4e-18 at x = 10)
    double s = 3617.0 / 8160.0;
    s = 1.0 / 12.0 - i2 * s;
    s = 691.0 / 32760.0 - i2 * s;
    s = 1.0 / 132.0 - i2 * s;
    s = 1.0 / 240.0 - i2 * s;
    s = 1.0 / 252.0 - i2 * s;
    s = 1.0 / 120.0 - i2 * s;
    s = 1.0 / 12.0 - i2 * s;
    return r + ((log(x) - 0.5 * i) - i2 * s);
}

// tables: [0, nu k) users, then the items
__global__ __launch_bounds__(kBlock) void hpf_elog_kernel(const double *__restrict__ Gs, const double *__restrict__ Gr,
                                                          const double *__restrict__ Ls, const double *__restrict__ Lr,
                                                          double *__restrict__ Lt, double *__restrict__ Lb, int64_t nu_k,
                                                          int64_t ni_k) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= nu_k + ni_k) return;
    const bool user = e < nu_k;
    const int64_t x = user ? e : e - nu_k;
    const double s = user ? Gs[x] : Ls[x], r = user ? Gr[x] : Lr[x];
    const double v = exp(hpf_digamma(s) - log(r));
    if (user) Lt[x] = v;
    else Lb[x] = v;
}

template <int G>
__device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kWave);
    return v;
}

struct HpfSumArgs {
    const int32_t *seg_row, *seg_len, *seg_dst;  // dst >= 0: accumulator row; < 0: partial slot -dst - 1
    const int64_t *seg_beg;
    int64_t n_seg;
    const int32_t *idx;      // the other side's id of a position
    const int32_t *pos;      // stored index j of a position (NULL: the position itself — the CSR)
    const float *val;        // [j]
    double *dk;              // [j] (DK = 1: written, DK = 2: read)
    const double *own, *other;   // Lt / Lb of this side and of the other
    double *acc, *part;      // part: [slot][k]
    int k;
};

// DK: 0 compute dk, 1 compute and store it, 2 read it
template <int G, int R, int DK>
__global__ __launch_bounds__(kBlock) void hpf_sum_kernel(const HpfSumArgs a) {
    static_assert(G == kWave || R == 1, "lane groups hold a whole row");
    const int lg = threadIdx.x & (G - 1);
    const int64_t grp = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const bool has = grp < a.n_seg;
    const int64_t s = has ? grp : a.n_seg - 1;
    const int32_t row = a.seg_row[s], dst = a.seg_dst[s];
    const int64_t beg = a.seg_beg[s];
    const int len = has ? a.seg_len[s] : 0;
    int maxlen = len;   // the trip count of the wave: every lane runs the cross-lane steps
    for (int o = G; o < kWave; o <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o, kWave));
    const int k = a.k;
    const double eps = 0x1p-52;   // pow(2, -52): cpp_hpf.cpp:43
    double own[R], sum[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int f = lg + G * c;
        own[c] = f < k ? a.own[(size_t)row * k + f] : 0.0;
        sum[c] = dst >= 0 ? kHpfPrior : 0.0;
    }
    for (int t0 = 0; t0 < maxlen; t0 += G) {
        // ---- G positions of the segment with one coalesced read per array ----
        const bool in = t0 + lg < len;
        const int64_t p = beg + t0 + lg;
        const int32_t ob = in ? a.idx[p] : 0;
        const int64_t jb = in ? (a.pos ? (int64_t)a.pos[p] : p) : 0;
        const float rb = in ? a.val[jb] : 0.f;
        double db = 1.0;
        if (DK == 2 && in) db = a.dk[jb];
        const int nb = min(G, maxlen - t0);
        for (int e = 0; e < nb; ++e) {
            const bool act = t0 + e < len;
            const int32_t o = __shfl(ob, e, G);
            const double x = (double)__shfl(rb, e, G);
            const double *po = a.other + (size_t)o * k;
            double P[R];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const int f = lg + G * c;
                P[c] = own[c] * ((act && f < k) ? po[f] : 0.0);
            }
            double dk;
            if (DK == 2) {
                dk = __shfl(db, e, G);
            } else {
                double d = P[0];
#pragma unroll
                for (int c = 1; c < R; ++c) d = d + P[c];
                dk = eps + group_sum_f64<G>(d);
                if (DK == 1 && act && lg == 0) a.dk[beg + t0 + e] = dk;   // the user side: the position is the stored index
            }
            if (act) {
#pragma unroll
                for (int c = 0; c < R; ++c) sum[c] = sum[c] + P[c] * x / dk;
            }
        }
    }
    if (has) {
        double *out = dst >= 0 ? a.acc + (size_t)dst * k : a.part + (size_t)(-dst - 1) * k;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int f = lg + G * c;
            if (f < k) out[f] = sum[c];
        }
    }
}

// the rows the plan split: ((prior + piece 0) + piece 1) + ...
__global__ __launch_bounds__(kBlock) void hpf_combine_kernel(const int32_t *__restrict__ c_row, const int32_t *__restrict__ c_slot,
                                                             const int32_t *__restrict__ c_n, int64_t n_comb,
                                                             const double *__restrict__ part, double *acc, int k) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_comb * k) return;
    const int64_t c = e / k;
    const int f = (int)(e - c * k);
    const double *p = part + (size_t)c_slot[c] * k;
    double v = kHpfPrior;
    for (int q = 0; q < c_n[c]; ++q) {
        v = v + p[f];
        p += k;
    }
    acc[(size_t)c_row[c] * k + f] = v;
}

// out[block][f] = sum over the block's rows of S[r,f] / Rt[r,f] (RATIO) or of S[r,f]: thread (sub, f) sums every nsub-th row
// of the block in ascending order, then a tree over the nsub partials.  kp = pow2 >= k, nsub = kBlock / kp.
template <bool RATIO>
__global__ __launch_bounds__(kBlock) void hpf_colsum_kernel(const double *__restrict__ S, const double *__restrict__ Rt, int64_t rows,
                                                            int k, int kp, int64_t rows_per_block, double *__restrict__ out) {
    __shared__ double lds[kBlock];
    const int t = threadIdx.x, f = t & (kp - 1), sub = t / kp, nsub = kBlock / kp;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    double acc = 0.0;
    if (f < k)
        for (int64_t r = r0 + sub; r < r1; r += nsub) {
            const size_t x = (size_t)r * k + f;
            acc = acc + (RATIO ? S[x] / Rt[x] : S[x]);
        }
    lds[t] = acc;
    __syncthreads();
    for (int o = nsub / 2; o > 0; o >>= 1) {
        if (sub < o) lds[t] = lds[t] + lds[t + o * kp];
        __syncthreads();
    }
    if (sub == 0 && f < k) out[(size_t)blockIdx.x * k + f] = lds[t];
}

// one lane group per row: update_rate: Rt[r,f] = ks / Kv[r] + col[f] (cpp_hpf.cpp:32-35); hier: Kv[r] = 0.3 + sum_f S / Rt (:7-19)
template <int G>
__global__ __launch_bounds__(kBlock) void hpf_rate_kernel(double *Rt, const double *__restrict__ S, const double *__restrict__ col,
                                                          double *Kv, int64_t rows, int k, double ks, int update_rate, int hier) {
    const int lg = threadIdx.x & (G - 1);
    const int64_t grp = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const bool has = grp < rows;
    const int64_t r = has ? grp : rows - 1;
    const double base = ks / Kv[r];
    double sum = 0.0;
    for (int f = lg; f < k; f += G) {
        const size_t x = (size_t)r * k + f;
        double rt;
        if (update_rate) {
            rt = base + col[f];
            if (has) Rt[x] = rt;
        } else {
            rt = Rt[x];
        }
        if (hier) sum = sum + S[x] / rt;
    }
    sum = group_sum_f64<G>(sum);
    if (hier && has && lg == 0) Kv[r] = kHpfPrior + sum;
}

__global__ __launch_bounds__(kBlock) void hpf_fill_kernel(double *p, int64_t n, double v) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < n) p[e] = v;
}

}  // namespace chip

// ---- host --------------------------------------------------------------------------------------------------------------
typedef void (*HpfSumKernel)(const HpfSumArgs);

template <int DK>
static HpfSumKernel pick_hpf_sum_kernel_t(int k) {
    if (k <= 8) return hpf_sum_kernel<8, 1, DK>;
    if (k <= 16) return hpf_sum_kernel<16, 1, DK>;
    if (k <= 32) return hpf_sum_kernel<32, 1, DK>;
    if (k <= 64) return hpf_sum_kernel<64, 1, DK>;
    if (k <= 128) return hpf_sum_kernel<64, 2, DK>;
    if (k <= 192) return hpf_sum_kernel<64, 3, DK>;
    return hpf_sum_kernel<64, 4, DK>;
}

static void hpf_launch_sums(cornac_hip_mf_t h, NmfPlan &pl, int side, int dk_form) {
    NmfSide &sd = pl.side[side];
    HpfSumArgs a;
    a.seg_row = sd.seg_row.p; a.seg_len = sd.seg_len.p; a.seg_dst = sd.seg_dst.p; a.seg_beg = sd.seg_beg.p; a.n_seg = sd.n_seg;
    a.idx = side == 0 ? h->nmf_cid.p : h->nmf_cuid.p;
    a.pos = side == 0 ? nullptr : h->nmf_perm.p;
    a.val = h->val.p; a.dk = h->hpf_dk.p;
    a.own = side == 0 ? h->hpf_Lt.p : h->hpf_Lb.p; a.other = side == 0 ? h->hpf_Lb.p : h->hpf_Lt.p;
    a.acc = side == 0 ? h->hpf_Gs.p : h->hpf_Ls.p; a.part = h->hpf_part.p; a.k = h->k;
    const int per_block = kBlock / nmf_group(h->k);
    const int64_t grid = (sd.n_seg + per_block - 1) / per_block;
    const HpfSumKernel kern = dk_form == 0 ? pick_hpf_sum_kernel_t<0>(h->k)
                                           : side == 0 ? pick_hpf_sum_kernel_t<1>(h->k) : pick_hpf_sum_kernel_t<2>(h->k);
    hipLaunchKernelGGL(kern, dim3((unsigned int)grid), dim3(kBlock), 0, h->stream, a);
    if (sd.n_comb > 0)
        hipLaunchKernelGGL(hpf_combine_kernel, dim3((unsigned int)((sd.n_comb * h->k + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           h->stream, sd.c_row.p, sd.c_slot.p, sd.c_n.p, sd.n_comb, h->hpf_part.p, a.acc, h->k);
}

static int64_t hpf_colsum_rows_per_block(int64_t rows, int kp) {
    return std::max<int64_t>((int64_t)(kBlock / kp) * 8, (rows + 1023) / 1024);
}

// hpf_col[f] = sum over the rows of S / Rt, in an order fixed by the shape alone
static void hpf_colsum(cornac_hip_mf_t h, const double *S, const double *Rt, int64_t rows) {
    int kp = 8;
    while (kp < h->k) kp <<= 1;
    const int64_t rpb = hpf_colsum_rows_per_block(rows, kp), blocks = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(hpf_colsum_kernel<true>, dim3((unsigned int)blocks), dim3(kBlock), 0, h->stream, S, Rt, rows, h->k, kp, rpb,
                       h->hpf_colpart.p);
    hipLaunchKernelGGL(hpf_colsum_kernel<false>, dim3(1), dim3(kBlock), 0, h->stream, (const double *)h->hpf_colpart.p,
                       (const double *)nullptr, blocks, h->k, kp, blocks, h->hpf_col.p);
}

static void hpf_rate(cornac_hip_mf_t h, double *Rt, const double *S, double *Kv, int64_t rows, double ks, int update_rate, int hier) {
    const int G = nmf_group(h->k);
    const dim3 grid((unsigned int)((rows * G + kBlock - 1) / kBlock)), block(kBlock);
#define HPF_RATE(GG) \
    hipLaunchKernelGGL(hpf_rate_kernel<GG>, grid, block, 0, h->stream, Rt, S, (const double *)h->hpf_col.p, Kv, rows, h->k, ks, update_rate, hier)
    switch (G) {
        case 8: HPF_RATE(8); break;
        case 16: HPF_RATE(16); break;
        case 32: HPF_RATE(32); break;
        default: HPF_RATE(64); break;
    }
#undef HPF_RATE
}

static void hpf_fill(cornac_hip_mf_t h, double *p, int64_t n, double v) {
    hipLaunchKernelGGL(hpf_fill_kernel, dim3((unsigned int)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, p, n, v);
}

static void hpf_elog(cornac_hip_mf_t h) {
    const int64_t eu = h->n_users * h->k, ei = h->n_items * h->k;
    hipLaunchKernelGGL(hpf_elog_kernel, dim3((unsigned int)((eu + ei + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                       (const double *)h->hpf_Gs.p, (const double *)h->hpf_Gr.p, (const double *)h->hpf_Ls.p,
                       (const double *)h->hpf_Lr.p, h->hpf_Lt.p, h->hpf_Lb.p, eu, ei);
}

extern "C" {

int cornac_hip_mf_hpf_set_tables(cornac_hip_mf_t h, const double *G_s, const double *G_r, const double *L_s, const double *L_r) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        REQUIRE(h->k <= kHpfMaxK, "HPF keeps a row's sums in registers: k = %d is above its limit of %d", h->k, kHpfMaxK);
        REQUIRE(G_s && G_r && L_s && L_r, "G_s, G_r, L_s and L_r are required");
        REQUIRE(h->n_users > 0 && h->n_items > 0, "HPF needs at least one user and one item");
        mf_check(h);
        const size_t nu = (size_t)h->n_users * h->k, ni = (size_t)h->n_items * h->k;
        h->hpf_Gs.ensure(nu); h->hpf_Gr.ensure(nu); h->hpf_Lt.ensure(nu); h->hpf_Kr.ensure((size_t)h->n_users);
        h->hpf_Ls.ensure(ni); h->hpf_Lr.ensure(ni); h->hpf_Lb.ensure(ni); h->hpf_Tr.ensure((size_t)h->n_items);
        h->hpf_col.ensure((size_t)h->k);
        h->hpf_colpart.ensure((size_t)1024 * h->k);
        h->hpf_Gs.upload(G_s, nu, h->stream); h->hpf_Gr.upload(G_r, nu, h->stream);
        h->hpf_Ls.upload(L_s, ni, h->stream); h->hpf_Lr.upload(L_r, ni, h->stream);
        hpf_fill(h, h->hpf_Kr.p, h->n_users, 1.0);
        hpf_fill(h, h->hpf_Tr.p, h->n_items, 1.0);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->hpf_set = true;
    });
}

int cornac_hip_mf_hpf_get_tables(cornac_hip_mf_t h, double *G_s, double *G_r, double *L_s, double *L_r, double *K_r, double *T_r) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(h->hpf_set, "cornac_hip_mf_hpf_set_tables has not been called on this handle");
        const size_t nu = (size_t)h->n_users * h->k, ni = (size_t)h->n_items * h->k;
        if (G_s) h->hpf_Gs.download(G_s, nu, h->stream);
        if (G_r) h->hpf_Gr.download(G_r, nu, h->stream);
        if (L_s) h->hpf_Ls.download(L_s, ni, h->stream);
        if (L_r) h->hpf_Lr.download(L_r, ni, h->stream);
        if (K_r) h->hpf_Kr.download(K_r, (size_t)h->n_users, h->stream);
        if (T_r) h->hpf_Tr.download(T_r, (size_t)h->n_items, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_mf_hpf_elog(cornac_hip_mf_t h, double *Lt, double *Lb) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(h->hpf_set, "cornac_hip_mf_hpf_elog before cornac_hip_mf_hpf_set_tables");
        hpf_elog(h);
        HIP_CHECK(hipGetLastError());
        if (Lt) h->hpf_Lt.download(Lt, (size_t)h->n_users * h->k, h->stream);
        if (Lb) h->hpf_Lb.download(Lb, (size_t)h->n_items * h->k, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_mf_hpf_fit(cornac_hip_mf_t h, int n_iters, int hierarchical) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        REQUIRE(h->hpf_set, "cornac_hip_mf_hpf_fit before cornac_hip_mf_hpf_set_tables");
        REQUIRE(n_iters >= 0, "n_iters must be >= 0");
        mf_check(h);
        if (!h->nmf_built)
            for (int64_t s = 1; s < h->nnz; ++s)
                REQUIRE(h->host_rid[(size_t)s] >= h->host_rid[(size_t)s - 1],
                        "HPF needs the ratings stored by user (rid non-decreasing: the CSR of the rating matrix); rating %lld breaks the order",
                        (long long)s);
        nmf_build(h);
        nmf_build_plan(h, CORNAC_HIP_MODE_HOGWILD);   // long rows split at kNmfSplit
        NmfPlan &pl = h->nmf_plan[CORNAC_HIP_MODE_HOGWILD];
        h->hpf_part.ensure(std::max<size_t>((size_t)pl.n_slots * h->k, 1));
        const int dk_form = prof_env_set("CORNAC_HIP_HPF_STORE_DK") ? 1 : 0;
        if (dk_form) h->hpf_dk.ensure(std::max<size_t>((size_t)h->nnz, 1));
        const int hier = hierarchical ? 1 : 0;
        const int64_t nu = h->n_users, ni = h->n_items;
        // cpp_hpf.cpp:222-223 / :154-155
        const double ks = hier ? kHpfPrior + h->k * kHpfPrior : kHpfPrior, ts = ks;
        const double *Gs = h->hpf_Gs.p, *Ls = h->hpf_Ls.p;
        // hpf.pyx:148-149 / :81-82: K_r = T_r = 1 on every call; cpp_hpf.cpp:231-234: hierarchical, from the tables
        hpf_fill(h, h->hpf_Kr.p, nu, 1.0);
        hpf_fill(h, h->hpf_Tr.p, ni, 1.0);
        if (hier) {
            hpf_rate(h, h->hpf_Gr.p, Gs, h->hpf_Kr.p, nu, ks, 0, 1);
            hpf_rate(h, h->hpf_Lr.p, Ls, h->hpf_Tr.p, ni, ts, 0, 1);
        }
        for (int it = 0; it < n_iters; ++it) {
            hpf_elog(h);                                             // 1
            hpf_launch_sums(h, pl, 0, dk_form);                      // 2
            hpf_colsum(h, Ls, h->hpf_Lr.p, ni);                      // 3: the L of the iteration before
            hpf_rate(h, h->hpf_Gr.p, Gs, h->hpf_Kr.p, nu, ks, 1, hier);   // 3 + 4
            hpf_launch_sums(h, pl, 1, dk_form);                      // 5
            hpf_colsum(h, Gs, h->hpf_Gr.p, nu);                      // 6: the new G
            hpf_rate(h, h->hpf_Lr.p, Ls, h->hpf_Tr.p, ni, ts, 1, hier);   // 6 + 7
            HIP_CHECK(hipGetLastError());
            h->hpf_group = nmf_group(h->k);
            h->hpf_rows_split = pl.rows_split;
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_mf_hpf_form(cornac_hip_mf_t h, int *group, int *rows_split) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        if (group) *group = h->hpf_group;
        if (rows_split) *rows_split = h->hpf_rows_split;
    });
}
}

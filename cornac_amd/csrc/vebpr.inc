// VEBPR (view-enhanced BPR) on the BPR handle — included at the end of bpr.hip.
//
// Replaces VEBPR._fit_sgd_viewloss (cornac/models/bpr/recom_vebpr.pyx:211-337): three sampler
// streams (purchase position, view draw, negative), membership tests against the purchase AND view
// rows, three clamped pairwise terms and a 4-row update; users without views fall back to a plain
// (bias-free, clamped) BPR step.  Same two modes as BPR: deterministic = bit-faithful mt19937
// streams + level schedule over the (u, i, v, j) row-conflict DAG, with the reference's mixed
// float/double expression types; hogwild = Philox sampling + row-wise fp32 atomics.

namespace chip {

__device__ __forceinline__ float clamp50(float x) { return x > 50.0f ? 50.0f : (x < -50.0f ? -50.0f : x); }

// stage 1: positive (u, i) per sample and whether the user has views (-> consumes a view draw)
__global__ __launch_bounds__(kBlock) void vebpr_det_stage1_kernel(const uint32_t *__restrict__ pos_draw, int64_t n,
                                                                  const int32_t *__restrict__ user_ids,
                                                                  const int32_t *__restrict__ indices,
                                                                  const int32_t *__restrict__ v_indptr,
                                                                  int32_t *__restrict__ su, int32_t *__restrict__ si,
                                                                  uint8_t *__restrict__ has_view) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t ii = pos_draw[s];
    const int32_t u = user_ids[ii];
    su[s] = u;
    si[s] = indices[ii];
    has_view[s] = v_indptr[u + 1] > v_indptr[u];
}

// stage 2: view item, negative item, skip test.  view_rank[s] = number of earlier samples with views
__global__ __launch_bounds__(kBlock) void vebpr_det_stage2_kernel(
    int64_t n, const int32_t *__restrict__ view_rank, const uint32_t *__restrict__ view_draw,
    const uint32_t *__restrict__ neg_draw, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    const int32_t *__restrict__ v_indptr, const int32_t *__restrict__ v_indices, int32_t *__restrict__ su,
    int32_t *__restrict__ sv, int32_t *__restrict__ sj, unsigned long long *__restrict__ counters) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool skip = false;
    if (s < n) {
        const int32_t u = su[s];
        const int32_t j = (int32_t)neg_draw[s];
        const int32_t nv = v_indptr[u + 1] - v_indptr[u];
        int32_t v = -1;
        skip = csr_row_contains(indices, indptr[u], indptr[u + 1], j);
        if (nv > 0) {
            v = v_indices[v_indptr[u] + (int32_t)(view_draw[view_rank[s]] % (uint32_t)nv)];
            skip = skip || csr_row_contains(v_indices, v_indptr[u], v_indptr[u + 1], j);
        }
        sv[s] = v;
        sj[s] = j;
        if (skip) su[s] = -1;
    }
    const unsigned long long m = __ballot(skip);
    if (lane_id() == 0 && m) atomicAdd(&counters[1], (unsigned long long)__popcll(m));
}

// T = float, or double for the float64 instantiation of the reference's fused-type function (recom_vebpr.pyx:219:
// float64 init_params train in double, every local of the step included)
template <int G, typename T>
__global__ __launch_bounds__(kBlock) void vebpr_det_level_kernel(const int32_t *__restrict__ ou,
                                                                 const int32_t *__restrict__ oi,
                                                                 const int32_t *__restrict__ ov,
                                                                 const int32_t *__restrict__ oj, int64_t off, int cnt,
                                                                 T *U, T *V, int k, T lr, T reg, T alpha,
                                                                 unsigned long long *__restrict__ counters) {
    const int gid = (blockIdx.x * kBlock + threadIdx.x) / G;
    const int lg = threadIdx.x & (G - 1);
    const bool active = gid < cnt;
    const int64_t t = off + (active ? gid : cnt - 1);
    const int32_t u = ou[t], i = oi[t], v = ov[t], j = oj[t];
    const bool has_v = v >= 0;
    T *user = U + (size_t)u * k, *item_i = V + (size_t)i * k, *item_j = V + (size_t)j * k;
    T *item_v = V + (size_t)(has_v ? v : i) * k;
    T x_uij = 0, x_uiv = 0, x_uvj = 0;
    for (int base = 0; base < k; base += G) {
        const int f = base + lg;
        T p1 = 0, p2 = 0, p3 = 0;
        if (f < k) {
            const T uf = user[f], a = item_i[f], b = item_v[f], c = item_j[f];
            p1 = uf * (a - c);
            p2 = uf * (a - b);
            p3 = uf * (b - c);
        }
        const int lim = min(G, k - base);
        x_uij = ordered_lane_sum_t<G>(x_uij, p1, lim);
        x_uiv = ordered_lane_sum_t<G>(x_uiv, p2, lim);
        x_uvj = ordered_lane_sum_t<G>(x_uvj, p3, lim);
    }
    const T hi = 50, lo = -50;
    x_uij = x_uij > hi ? hi : (x_uij < lo ? lo : x_uij);
    x_uiv = x_uiv > hi ? hi : (x_uiv < lo ? lo : x_uiv);
    x_uvj = x_uvj > hi ? hi : (x_uvj < lo ? lo : x_uvj);
    const T delta_ij = sigmoid_neg_exact_t(x_uij), delta_iv = sigmoid_neg_exact_t(x_uiv),
            delta_vj = sigmoid_neg_exact_t(x_uvj);
    const T half = (T)0.5;
    bool ok;
    if (!has_v) {
        ok = delta_ij < half;
        if (active) {
            for (int f = lg; f < k; f += G) {
                const T u_old = user[f], i_old = item_i[f], j_old = item_j[f];
                T nu = u_old, ni = i_old, nj = j_old;
                nu -= lr * (-delta_ij * (i_old - j_old) + reg * u_old);
                ni -= lr * (-delta_ij * u_old + reg * i_old);
                nj -= lr * (delta_ij * u_old + reg * j_old);
                user[f] = nu;
                item_i[f] = ni;
                item_j[f] = nj;
            }
        }
    } else {
        ok = delta_ij < half && delta_iv < half && delta_vj < half;
        if (active) {
            for (int f = lg; f < k; f += G) {
                const T u_old = user[f], i_old = item_i[f], v_old = item_v[f], j_old = item_j[f];
                T nu = u_old, ni = i_old, nv = v_old, nj = j_old;
                // `1.0` is a double literal in the reference's generated C: these terms are evaluated in double
                nu -= lr * (-delta_ij * (i_old - j_old) - alpha * delta_iv * (i_old - v_old) -
                            (1.0 - alpha) * delta_vj * (v_old - j_old) + reg * u_old);
                ni -= lr * (-delta_ij * u_old - alpha * delta_iv * u_old + reg * i_old);
                nv -= lr * (alpha * delta_iv * u_old - (1.0 - alpha) * delta_vj * u_old + reg * v_old);
                nj -= lr * (delta_ij * u_old + (1.0 - alpha) * delta_vj * u_old + reg * j_old);
                user[f] = nu;
                item_i[f] = ni;
                item_v[f] = nv;
                item_j[f] = nj;
            }
        }
    }
    const unsigned long long m = __ballot(active && lg == 0 && ok);
    if (lane_id() == 0 && m) atomicAdd(&counters[0], (unsigned long long)__popcll(m));
}

struct VeArgs {
    const int32_t *user_ids, *indices, *indptr, *v_indptr, *v_indices;
    float *U, *V;
    unsigned long long *counters;
    int64_t n;
    uint64_t s_begin, seed;
    uint32_t epoch, n_pos, th_pos, n_items;
    int k;
    float lr, reg, alpha;
    // user-row ownership (bpr.hip build_ownership): wave w draws its positives from own_u / own_i[wave_ptr[w] ..
    // wave_ptr[w+1]); own_u < 0 encodes a shared (heavy) user as ~u
    const int32_t *own_u, *own_i;
    const int64_t *wave_ptr;
};

// hogwild: one wave samples 64 (u, i, v, j) quadruples (lane-parallel), then processes the valid ones
// TPW at a time with G lanes per row (row-wise layout: whole-line gathers and fp32-atomic scatters).
// OWNED (G == 64: one quadruple per wave step): every wave owns a fixed set of users for the launch and draws its
// positives only from their interactions (one slice per wave, |slice| samples per epoch), so an exclusive user's row
// has ONE writer: plain load / store instead of an fp32 atomic per line, as in bpr_hogwild_rowwise_kernel.  Item rows
// (three per quadruple) keep the atomics.
template <int G, int R, bool OWNED>
__global__ __launch_bounds__(kBlock) void vebpr_hogwild_kernel(const VeArgs a) {
    static_assert(!OWNED || G == kWave, "ownership needs one quadruple per wave step");
    __shared__ int32_t stage[kWavesPerBlock][4][kWave];
    constexpr int TPW = kWave / G;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int grp = lane / G, lg = lane & (G - 1);
    const int64_t total_waves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t wave_id = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    int64_t n_tiles = (a.n + kWave - 1) / kWave, tile0 = wave_id, tile_step = total_waves;
    int64_t own_base = 0;
    uint32_t own_len = 1, own_th = 0;
    if (OWNED) {
        own_base = a.wave_ptr[wave_id];
        own_len = (uint32_t)(a.wave_ptr[wave_id + 1] - own_base);
        n_tiles = (own_len + kWave - 1) / kWave;   // own_len == 0: no tiles
        tile0 = 0;
        tile_step = 1;
        own_th = own_len ? lemire_thresh(own_len) : 0;
    }
    unsigned int n_correct = 0, n_skipped = 0;
    for (int64_t tile = tile0; tile < n_tiles; tile += tile_step) {
        const int64_t local = tile * kWave + lane;
        const bool in_range = OWNED ? local < (int64_t)own_len : local < a.n;
        const uint64_t s = a.s_begin + (uint64_t)(in_range ? local : 0);
        uint32_t w[4];
        int32_t u, i, u_enc;
        if (OWNED) {
            philox4x32_10((uint32_t)s, (uint32_t)wave_id, a.epoch, 3u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
            const uint32_t r = lemire_bounded2(w[0], w[1], own_len, own_th);
            u_enc = a.own_u[own_base + r];
            i = a.own_i[own_base + r];
            u = u_enc < 0 ? ~u_enc : u_enc;
        } else {
            philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), a.epoch, 2u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
            const uint32_t ii = lemire_bounded2(w[0], w[1], a.n_pos, a.th_pos);
            u = a.user_ids[ii];
            i = a.indices[ii];
            u_enc = ~u;   // not owned: the atomic path
        }
        const int32_t j = (int32_t)(((uint64_t)w[3] * a.n_items) >> 32);
        const int32_t v0 = a.v_indptr[u], nv = a.v_indptr[u + 1] - v0;
        int32_t v = -1;
        bool skip = csr_row_contains(a.indices, a.indptr[u], a.indptr[u + 1], j);
        if (nv > 0) {
            v = a.v_indices[v0 + (int32_t)(((uint64_t)w[2] * (uint32_t)nv) >> 32)];
            skip = skip || csr_row_contains(a.v_indices, v0, v0 + nv, j);
        }
        const bool valid = in_range && !skip;
        const unsigned long long mask = __ballot(valid);
        n_skipped += (in_range && !valid) ? 1u : 0u;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            stage[wave][0][pos] = OWNED ? u_enc : u;
            stage[wave][1][pos] = i;
            stage[wave][2][pos] = v;
            stage[wave][3][pos] = j;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nvalid = __popcll(mask);
        for (int b = 0; b < nvalid; b += TPW) {
            const int slot = b + grp;
            const bool act = slot < nvalid;
            const int sl = act ? slot : b;
            int32_t tu = stage[wave][0][sl];
            const int32_t ti = stage[wave][1][sl], tv = stage[wave][2][sl], tj = stage[wave][3][sl];
            bool exclusive = false;
            if (OWNED) {
                tu = __builtin_amdgcn_readfirstlane(tu);   // one quadruple per wave step: wave-uniform
                exclusive = tu >= 0;
                if (tu < 0) tu = ~tu;
            }
            const bool has_v = tv >= 0;
            float *pu = a.U + (size_t)tu * a.k + lg, *pi = a.V + (size_t)ti * a.k + lg;
            float *pv = a.V + (size_t)(has_v ? tv : ti) * a.k + lg, *pj = a.V + (size_t)tj * a.k + lg;
            float uf[R], vi[R], vv[R], vj[R];
            float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool inb = lg + G * r < a.k;
                uf[r] = inb ? __builtin_nontemporal_load(pu + G * r) : 0.f;
                vi[r] = inb ? __builtin_nontemporal_load(pi + G * r) : 0.f;
                vv[r] = inb ? __builtin_nontemporal_load(pv + G * r) : 0.f;
                vj[r] = inb ? __builtin_nontemporal_load(pj + G * r) : 0.f;
                s1 += uf[r] * (vi[r] - vj[r]);
                s2 += uf[r] * (vi[r] - vv[r]);
                s3 += uf[r] * (vv[r] - vj[r]);
            }
            const float d_ij = sigmoid_neg_fast(clamp50(group_sum<G>(s1)));
            const float d_iv = has_v ? sigmoid_neg_fast(clamp50(group_sum<G>(s2))) : 0.f;
            const float d_vj = has_v ? sigmoid_neg_fast(clamp50(group_sum<G>(s3))) : 0.f;
            const float al = has_v ? a.alpha : 0.f, be = has_v ? 1.0f - a.alpha : 0.f;
            if (act) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (lg + G * r < a.k) {
                        const float u0 = uf[r];
                        const float du = -a.lr * (-d_ij * (vi[r] - vj[r]) - al * d_iv * (vi[r] - vv[r]) -
                                                  be * d_vj * (vv[r] - vj[r]) + a.reg * u0);
                        if (OWNED && exclusive) pu[G * r] = u0 + du;   // the row's only writer
                        else atomic_add_f32(pu + G * r, du);
                        atomic_add_f32(pi + G * r, -a.lr * (-d_ij * u0 - al * d_iv * u0 + a.reg * vi[r]));
                        if (has_v) atomic_add_f32(pv + G * r, -a.lr * (al * d_iv * u0 - be * d_vj * u0 + a.reg * vv[r]));
                        atomic_add_f32(pj + G * r, -a.lr * (d_ij * u0 + be * d_vj * u0 + a.reg * vj[r]));
                    }
                }
                if (lg == 0) n_correct += (d_ij < .5f && (!has_v || (d_iv < .5f && d_vj < .5f))) ? 1u : 0u;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_correct += __shfl_xor(n_correct, o, kWave);
        n_skipped += __shfl_xor(n_skipped, o, kWave);
    }
    if (lane == 0) {
        if (n_correct) atomicAdd(&a.counters[0], (unsigned long long)n_correct);
        if (n_skipped) atomicAdd(&a.counters[1], (unsigned long long)n_skipped);
    }
}

}  // namespace chip

using namespace chip;

template <int G>
static void launch_vebpr_level(cornac_hip_bpr_t h, const int32_t *ou, const int32_t *oi, const int32_t *ov,
                               const int32_t *oj, int64_t off, int cnt, double lr, double reg, double alpha) {
    const int groups_per_block = kBlock / G;
    const int grid = (cnt + groups_per_block - 1) / groups_per_block;
    if (h->f64)
        hipLaunchKernelGGL((vebpr_det_level_kernel<G, double>), dim3(grid), dim3(kBlock), 0, h->stream, ou, oi, ov, oj, off, cnt,
                           h->U64.p, h->V64.p, h->k, lr, reg, alpha, h->counters.p);
    else
        hipLaunchKernelGGL((vebpr_det_level_kernel<G, float>), dim3(grid), dim3(kBlock), 0, h->stream, ou, oi, ov, oj, off, cnt,
                           h->U.p, h->V.p, h->k, (float)lr, (float)reg, (float)alpha, h->counters.p);
}

static void vebpr_epoch_deterministic(cornac_hip_bpr_t h, double lr, double reg, double alpha) {
    REQUIRE(h->mt_seeded && h->view_seeded, "deterministic VEBPR needs the three mt19937 streams seeded");
    const int64_t nnz = h->nnz;
    const int64_t chunk = std::min(nnz, kDetChunk);
    h->draws.ensure((size_t)3 * chunk);
    h->trip.ensure((size_t)8 * chunk);
    h->h_trip.ensure((size_t)8 * chunk);
    h->view_rank.ensure((size_t)chunk);
    h->has_view.ensure((size_t)chunk);
    std::vector<uint8_t> flags((size_t)chunk);
    std::vector<int32_t> ranks((size_t)chunk);
    const int G = pow2_group(h->k);
    for (int64_t c0 = 0; c0 < nnz; c0 += chunk) {
        const int64_t n = std::min(chunk, nnz - c0);
        Timer t_s;
        uint32_t *d_pos = h->draws.p, *d_neg = d_pos + chunk, *d_view = d_neg + chunk;
        {
            const int st[2] = {0, 1};
            const uint64_t his[2] = {(uint64_t)nnz - 1, (uint64_t)h->n_items - 1};
            const int64_t needs[2] = {n, n};
            uint32_t *outs[2] = {d_pos, d_neg};
            mt_draw(h, 2, st, his, needs, outs);
        }
        int32_t *su = h->trip.p, *si = su + chunk, *sv = si + chunk, *sj = sv + chunk;
        int32_t *ou = sj + chunk, *oi = ou + chunk, *ov = oi + chunk, *oj = ov + chunk;
        const unsigned g1 = (unsigned)((n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(vebpr_det_stage1_kernel, dim3(g1), dim3(kBlock), 0, h->stream, d_pos, n, h->user_ids.p,
                           h->indices.p, h->v_indptr.p, su, si, h->has_view.p);
        HIP_CHECK(hipMemcpyAsync(flags.data(), h->has_view.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        // the view stream is consumed only by samples whose user has views, in sample order
        int32_t n_view = 0;
        for (int64_t s = 0; s < n; ++s) {
            ranks[(size_t)s] = n_view;
            n_view += flags[(size_t)s];
        }
        HIP_CHECK(hipMemcpyAsync(h->view_rank.p, ranks.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        {
            const int st = 2;
            const uint64_t hi = (uint64_t)h->n_items - 1;
            const int64_t need = n_view;
            uint32_t *o = d_view;
            mt_draw(h, 1, &st, &hi, &need, &o);
        }
        hipLaunchKernelGGL(vebpr_det_stage2_kernel, dim3(g1), dim3(kBlock), 0, h->stream, n, h->view_rank.p, d_view,
                           d_neg, h->indptr.p, h->indices.p, h->v_indptr.p, h->v_indices.p, su, sv, sj, h->counters.p);
        HIP_CHECK(hipGetLastError());
        int32_t *hs = h->h_trip.p;
        HIP_CHECK(hipMemcpyAsync(hs, su, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(hs + chunk, si, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(hs + 2 * chunk, sv, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipMemcpyAsync(hs + 3 * chunk, sj, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->timing[0] += t_s.ms();
        Timer t_l;
        int32_t *ho = hs + 4 * chunk;
        build_level_schedule4(hs, hs + chunk, hs + 2 * chunk, hs + 3 * chunk, n, h->total_users, h->total_items, ho,
                              ho + chunk, ho + 2 * chunk, ho + 3 * chunk, h->sched, h->lvl_u, h->lvl_i, h->level);
        h->timing[1] += t_l.ms();
        Timer t_k;
        const int64_t na = h->sched.n_active;
        if (na > 0) {
            HIP_CHECK(hipMemcpyAsync(ou, ho, (size_t)na * 4, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(oi, ho + chunk, (size_t)na * 4, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(ov, ho + 2 * chunk, (size_t)na * 4, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(oj, ho + 3 * chunk, (size_t)na * 4, hipMemcpyHostToDevice, h->stream));
        }
        const std::vector<int64_t> &lp = h->sched.level_ptr;
        for (size_t l = 1; l + 1 < lp.size(); ++l) {
            const int64_t off = lp[l];
            const int cnt = (int)(lp[l + 1] - lp[l]);
            if (cnt <= 0) continue;
            switch (G) {
                case 4: launch_vebpr_level<4>(h, ou, oi, ov, oj, off, cnt, lr, reg, alpha); break;
                case 8: launch_vebpr_level<8>(h, ou, oi, ov, oj, off, cnt, lr, reg, alpha); break;
                case 16: launch_vebpr_level<16>(h, ou, oi, ov, oj, off, cnt, lr, reg, alpha); break;
                case 32: launch_vebpr_level<32>(h, ou, oi, ov, oj, off, cnt, lr, reg, alpha); break;
                default: launch_vebpr_level<64>(h, ou, oi, ov, oj, off, cnt, lr, reg, alpha); break;
            }
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->timing[2] += t_k.ms();
    }
}

// user-row ownership: one quadruple per wave step (k > 32) and at least one 64-sample tile per wave and epoch — the
// rule of hogwild_uses_ownership (bpr.hip)
static bool vebpr_uses_ownership(cornac_hip_bpr_t h, bool opt_out) {
    if (opt_out || h->k <= 32 || h->k > 256) return false;
    return h->nnz >= (int64_t)device_info(h->device).cus * 6 * kWavesPerBlock * kWave;
}

static void vebpr_epoch_hogwild(cornac_hip_bpr_t h, float lr, float reg, float alpha, bool no_ownership) {
    REQUIRE(h->hog_seeded, "hogwild mode needs cornac_hip_bpr_seed_hogwild first");
    const DeviceInfo &di = device_info(h->device);
    VeArgs a;
    a.user_ids = h->user_ids.p; a.indices = h->indices.p; a.indptr = h->indptr.p;
    a.v_indptr = h->v_indptr.p; a.v_indices = h->v_indices.p;
    a.U = h->U.p; a.V = h->V.p; a.counters = h->counters.p;
    a.n = h->nnz; a.s_begin = 0; a.seed = h->hog_seed; a.epoch = h->hog_epoch++;
    a.n_pos = (uint32_t)h->nnz; a.th_pos = lemire_thresh(a.n_pos); a.n_items = (uint32_t)h->n_items;
    a.k = h->k; a.lr = lr; a.reg = reg; a.alpha = alpha;
    const int64_t n_tiles = (a.n + kWave - 1) / kWave;
    const int64_t want = (n_tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)di.cus * 6));
    const int k = h->k;
    REQUIRE(k <= 256, "VEBPR hogwild supports k <= 256");
    const bool owned = vebpr_uses_ownership(h, no_ownership);
    a.own_u = nullptr; a.own_i = nullptr; a.wave_ptr = nullptr;
    if (owned) {
        grid = di.cus * 6;   // every wave of the grid owns a slice: the grid is the ownership table's width
        build_ownership(h, (int64_t)grid * kWavesPerBlock);
        a.own_u = h->own_u.p; a.own_i = h->own_i.p; a.wave_ptr = h->wave_ptr.p;
    }
    h->vebpr_owned = owned;
    dim3 g(grid), b(kBlock);
    if (k <= 4) hipLaunchKernelGGL((vebpr_hogwild_kernel<4, 1, false>), g, b, 0, h->stream, a);
    else if (k <= 8) hipLaunchKernelGGL((vebpr_hogwild_kernel<8, 1, false>), g, b, 0, h->stream, a);
    else if (k <= 16) hipLaunchKernelGGL((vebpr_hogwild_kernel<16, 1, false>), g, b, 0, h->stream, a);
    else if (k <= 32) hipLaunchKernelGGL((vebpr_hogwild_kernel<32, 1, false>), g, b, 0, h->stream, a);
    else if (k <= 64 && owned) hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 1, true>), g, b, 0, h->stream, a);
    else if (k <= 64) hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 1, false>), g, b, 0, h->stream, a);
    else if (k <= 128 && owned) hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 2, true>), g, b, 0, h->stream, a);
    else if (k <= 128) hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 2, false>), g, b, 0, h->stream, a);
    else if (owned) hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 4, true>), g, b, 0, h->stream, a);
    else hipLaunchKernelGGL((vebpr_hogwild_kernel<64, 4, false>), g, b, 0, h->stream, a);
    HIP_CHECK(hipGetLastError());
}

extern "C" {

int cornac_hip_bpr_set_views(cornac_hip_bpr_t h, const int32_t *view_indptr, const int32_t *view_indices,
                             int64_t nnz_view) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(view_indptr != nullptr && nnz_view >= 0, "bad view matrix");
        REQUIRE(view_indptr[0] == 0 && (int64_t)view_indptr[h->n_users] == nnz_view, "view indptr does not match nnz");
        for (int64_t u = 0; u < h->n_users; ++u)
            for (int32_t p = view_indptr[u]; p < view_indptr[u + 1]; ++p) {
                REQUIRE(view_indices[p] >= 0 && view_indices[p] < h->n_items, "view column index out of range");
                REQUIRE(p == view_indptr[u] || view_indices[p] > view_indices[p - 1], "view row %lld is not sorted",
                        (long long)u);
            }
        h->v_indptr.alloc((size_t)h->n_users + 1);
        h->v_indices.alloc((size_t)std::max<int64_t>(nnz_view, 1));
        h->v_indptr.upload(view_indptr, (size_t)h->n_users + 1, h->stream);
        if (nnz_view > 0) h->v_indices.upload(view_indices, (size_t)nnz_view, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->has_views = true;
    });
}

int cornac_hip_bpr_seed_view_stream(cornac_hip_bpr_t h, uint32_t mt_seed_view) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(h->mt_seeded, "seed the positive/negative streams first (cornac_hip_bpr_seed_mt19937)");
        std::vector<uint32_t> st(MT_N);
        mt_init_genrand(mt_seed_view, st.data());
        const int32_t idx = MT_N;
        HIP_CHECK(hipMemcpyAsync(h->mt_state.p + 2 * MT_N, st.data(), MT_N * 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->mt_idx.p + 2, &idx, 4, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->view_seeded = true;
    });
}

int cornac_hip_vebpr_fit_epochs(cornac_hip_bpr_t h, int n_epochs, float lr, float reg, float alpha, int mode,
                                int64_t *correct, int64_t *skipped) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(!h->f64, "the handle holds float64 tables (VEBPR trains float32 tables here)");
        REQUIRE(h->has_views, "cornac_hip_bpr_set_views has not been called");
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        const bool no_ownership = (mode & CORNAC_HIP_VEBPR_NO_OWNERSHIP) != 0;
        mode &= ~CORNAC_HIP_VEBPR_NO_OWNERSHIP;
        REQUIRE(mode == CORNAC_HIP_MODE_DETERMINISTIC || mode == CORNAC_HIP_MODE_HOGWILD, "unknown mode %d", mode);
        if (correct) *correct = 0;
        if (skipped) *skipped = 0;
        for (double &t : h->timing) t = 0;
        Timer total;
        HIP_CHECK(hipMemsetAsync(h->counters.p, 0, 2 * sizeof(unsigned long long), h->stream));
        for (int e = 0; e < n_epochs; ++e) {
            if (mode == CORNAC_HIP_MODE_DETERMINISTIC) vebpr_epoch_deterministic(h, lr, reg, alpha);
            else vebpr_epoch_hogwild(h, lr, reg, alpha, no_ownership);
        }
        fetch_counters(h, correct, skipped);
        h->timing[3] = total.ms();
    });
}

int cornac_hip_vebpr_fit_epochs_f64(cornac_hip_bpr_t h, int n_epochs, double lr, double reg, double alpha, int64_t *correct,
                                    int64_t *skipped) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(h->f64, "set float64 tables first (cornac_hip_bpr_set_factors_f64; the bias table is not used)");
        REQUIRE(h->has_views, "cornac_hip_bpr_set_views has not been called");
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        if (correct) *correct = 0;
        if (skipped) *skipped = 0;
        for (double &t : h->timing) t = 0;
        Timer total;
        HIP_CHECK(hipMemsetAsync(h->counters.p, 0, 2 * sizeof(unsigned long long), h->stream));
        for (int e = 0; e < n_epochs; ++e) vebpr_epoch_deterministic(h, lr, reg, alpha);
        fetch_counters(h, correct, skipped);
        h->timing[3] = total.ms();
    });
}

int cornac_hip_vebpr_hogwild_form(cornac_hip_bpr_t h, int *owned) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(owned != nullptr, "owned is NULL");
        *owned = h->vebpr_owned ? 1 : 0;
    });
}
}

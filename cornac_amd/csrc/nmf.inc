// NMF: multiplicative-update factorisation in float32 — included at the end of mf.hip, on the MF handle.
//
// Replaces NMF._fit_sgd (cornac/models/nmf/recom_nmf.pyx:182-267).  Per epoch, with U and V frozen, for every rating j of
// the CSR (stored by user):
//     r_pred = ((mu + Bu[u]) + Bi[i]) + U[u,0] V[i,0] + ... + U[u,k-1] V[i,k-1]          (index order)
//     error  = r - r_pred
//     use_bias:  Bu[u] += lr (error - lambda_bu Bu[u]);  Bi[i] += lr (error - lambda_bi Bi[i])     (:236-238, in stored order)
//     U_num[u,f] += r V[i,f];  U_den[u,f] += r_pred V[i,f];  V_num[i,f] += r U[u,f];  V_den[i,f] += r_pred U[u,f]   (:241-245)
// then  U_den[u,f] += count_u lambda_u U[u,f] + eps;  U[u,f] *= U_num[u,f] / U_den[u,f]   for all users, then the items
// (:248-259).  Every operation is a separately rounded float32 + - * / with contraction off.
//
//   nmf_bias_level_kernel  use_bias: one launch per level of the row-conflict schedule (mf_build_schedule's levels) —
//                          below 4096 ratings and after a refused cooperative launch.  Also the plain r_pred pass of
//                          k > 256 without biases (one launch over all ratings).
//   nmf_bias_chain_kernel  use_bias, from 4096 ratings: the dataflow driver of chain.h (one persistent launch; the
//                          protocol is explained there), users owned — a user's ratings are adjacent in the CSR and its Bu stays with one wave
//                          — the item bias handed over by version counters with system-scope loads and stores.  U and V
//                          are frozen, so the per-rating body is the serial dot plus scalars, any k; it stores r_pred[j].
//                          Sequential-exact in both modes.
//   nmf_sum_kernel         one lane group of G = pow2 >= k lanes (8..64; 64 / G rows per wave, as pmf.inc packs ratings)
//                          owns a SEGMENT of one row and walks it in ascending position, its 2 x k sums in registers
//                          (k <= 256: four slices of 64).  The user side (CSR) computes r_pred from the one read of
//                          each V row it needs anyway and stores it (no biases) or reads the bias pass's; the item side
//                          walks a CSC permutation built once per handle (ascending stored position inside an item)
//                          and reads r_pred[j] back.
//                            deterministic: a segment is a whole row, the dot product is serial in f  ->  the
//                                           reference's single-thread bits;
//                            hogwild:       rows longer than kNmfSplit are cut into segments of kNmfSplit ratings
//                                           whose partial sums nmf_combine_kernel adds in ascending order, the dot
//                                           product is a butterfly — exact sums in another, FIXED order: the same
//                                           bits run to run, one owner per accumulator row, no float atomics.
//   nmf_sum_generic_kernel k > 256: the same walk by one wave with the sums in memory (its own output rows).
//   nmf_update_kernel      the element-wise update and the regulariser's share of the loss.
// loss[epoch] = sum error^2 + lambda_u sum U^2 + lambda_v sum V^2 over the pre-update tables: float32 terms, summed in
// double in another order than the reference's float accumulator (compared with a tolerance).

namespace chip {

constexpr int kNmfSplit = 256;     // hogwild: ratings per segment of a long row
constexpr int kNmfFastK = 256;     // sums in registers up to here

struct NmfSumArgs {
    const int32_t *seg_row, *seg_len, *seg_dst;  // dst >= 0: accumulator row; < 0: partial slot -dst - 1
    const int64_t *seg_beg;                      // first position of the segment on this side
    int64_t n_seg;
    const int32_t *idx;      // the other side's id of a position
    const int32_t *pos;      // stored index j of a position (NULL: the position itself — the CSR)
    const float *val;        // [j]
    float *pred;             // [j] r_pred: written by the PRED form, read by the others
    const float *own, *other, *b_own, *b_other;
    float mu;
    float *acc_num, *acc_den, *part;   // part: [slot][2][k]
    double *loss_acc;
    int k;
};

template <int G, int R, bool ORDERED, bool PRED>
__global__ __launch_bounds__(kBlock) void nmf_sum_kernel(const NmfSumArgs a) {
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
    float own[R], num[R], den[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int f = lg + G * c;
        own[c] = f < k ? a.own[(size_t)row * k + f] : 0.f;
        num[c] = 0.f;
        den[c] = 0.f;
    }
    const float mub = PRED ? a.mu + a.b_own[row] : 0.f;
    double e2 = 0.0;
    for (int t0 = 0; t0 < maxlen; t0 += G) {
        // ---- G positions of the segment with one coalesced read per array ----
        const bool in = t0 + lg < len;
        const int64_t p = beg + t0 + lg;
        const int32_t ob = in ? a.idx[p] : 0;
        const int64_t jb = in ? (a.pos ? (int64_t)a.pos[p] : p) : 0;
        const float rb = in ? a.val[jb] : 0.f;
        const float xb = in ? (PRED ? a.b_other[ob] : a.pred[jb]) : 0.f;   // the other side's bias | r_pred
        const int nb = min(G, maxlen - t0);
        for (int e = 0; e < nb; ++e) {
            const bool act = t0 + e < len;
            const int32_t o = __shfl(ob, e, G);
            const float r = __shfl(rb, e, G), x = __shfl(xb, e, G);
            const float *po = a.other + (size_t)o * k;
            float v[R];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const int f = lg + G * c;
                v[c] = (act && f < k) ? po[f] : 0.f;
            }
            float pred = x;
            if (PRED) {
                pred = mub + x;
                if (ORDERED) {
#pragma unroll
                    for (int c = 0; c < R; ++c)
                        if (G * c < k) pred = ordered_lane_sum<G>(pred, own[c] * v[c], min(G, k - G * c));
                } else {
                    float d = own[0] * v[0];
#pragma unroll
                    for (int c = 1; c < R; ++c) d = d + own[c] * v[c];
                    pred = pred + group_sum<G>(d);
                }
                if (act && lg == 0) {
                    a.pred[beg + t0 + e] = pred;
                    const float err = r - pred;
                    e2 += (double)(err * err);
                }
            }
            if (act) {
#pragma unroll
                for (int c = 0; c < R; ++c) {
                    num[c] = num[c] + r * v[c];
                    den[c] = den[c] + pred * v[c];
                }
            }
        }
    }
    if (has) {
        float *on = dst >= 0 ? a.acc_num + (size_t)dst * k : a.part + (size_t)(-dst - 1) * 2 * k;
        float *od = dst >= 0 ? a.acc_den + (size_t)dst * k : on + k;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int f = lg + G * c;
            if (f < k) {
                on[f] = num[c];
                od[f] = den[c];
            }
        }
    }
    if (PRED) {
        const double l = wave_sum_f64(e2);
        if (lane_id() == 0 && l != 0.0) atomicAdd(a.loss_acc, l);
    }
}

// k > 256: one wave per segment, the sums in the segment's own output rows; r_pred is read
__global__ __launch_bounds__(kBlock) void nmf_sum_generic_kernel(const NmfSumArgs a) {
    const int lane = lane_id();
    const int64_t s = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
    if (s >= a.n_seg) return;
    const int32_t dst = a.seg_dst[s];
    const int64_t beg = a.seg_beg[s];
    const int len = a.seg_len[s], k = a.k;
    float *on = dst >= 0 ? a.acc_num + (size_t)dst * k : a.part + (size_t)(-dst - 1) * 2 * k;
    float *od = dst >= 0 ? a.acc_den + (size_t)dst * k : on + k;
    for (int f = lane; f < k; f += kWave) {
        on[f] = 0.f;
        od[f] = 0.f;
    }
    for (int t = 0; t < len; ++t) {
        const int64_t p = beg + t;
        const int32_t o = a.idx[p];
        const int64_t j = a.pos ? (int64_t)a.pos[p] : p;
        const float r = a.val[j], pred = a.pred[j];
        const float *po = a.other + (size_t)o * k;
        for (int f = lane; f < k; f += kWave) {   // a lane reads and writes its own factors only
            const float v = po[f];
            on[f] = on[f] + r * v;
            od[f] = od[f] + pred * v;
        }
    }
}

// the rows the hogwild plan split: partial sums added in ascending segment order
__global__ __launch_bounds__(kBlock) void nmf_combine_kernel(const int32_t *__restrict__ c_row, const int32_t *__restrict__ c_slot,
                                                             const int32_t *__restrict__ c_n, int64_t n_comb,
                                                             const float *__restrict__ part, float *acc_num, float *acc_den, int k) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_comb * k) return;
    const int64_t c = e / k;
    const int f = (int)(e - c * k);
    const float *p = part + (size_t)c_slot[c] * 2 * k;
    float num = p[f], den = p[k + f];
    for (int q = 1; q < c_n[c]; ++q) {
        p += 2 * k;
        num = num + p[f];
        den = den + p[k + f];
    }
    acc_num[(size_t)c_row[c] * k + f] = num;
    acc_den[(size_t)c_row[c] * k + f] = den;
}

// recom_nmf.pyx:248-259: den += count lambda T + eps (left to right, count converted to float), T *= num / den
__global__ __launch_bounds__(kBlock) void nmf_update_kernel(float *T, const float *__restrict__ num, const float *__restrict__ den,
                                                            const int64_t *__restrict__ ptr, int64_t n_rows, int k, float lambda,
                                                            double *loss_acc) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double reg = 0.0;
    if (e < n_rows * k) {
        const int64_t row = e / k;
        const float cnt = (float)(ptr[row + 1] - ptr[row]);
        const float eps = (float)1e-9;
        const float x = T[e];
        reg = (double)(lambda * x * x);
        float d = den[e];
        d = d + (cnt * lambda * x + eps);
        T[e] = x * (num[e] / d);
    }
    const double l = wave_sum_f64(reg);
    if (lane_id() == 0 && l != 0.0) atomicAdd(loss_acc, l);
}

// one rating per lane group: r_pred with the serial dot, stored; use_bias: the two bias steps.  lpos: the stored index of
// a schedule position (NULL: the position itself)
template <int G>
__global__ __launch_bounds__(kBlock) void nmf_bias_level_kernel(const int32_t *__restrict__ lpos, const int32_t *__restrict__ uid,
                                                                const int32_t *__restrict__ cid, const float *__restrict__ val,
                                                                int64_t off, int cnt, const float *__restrict__ U,
                                                                const float *__restrict__ V, float *Bu, float *Bi, float *pred_out,
                                                                int k, float lr, float lbu, float lbi, float mu, int use_bias,
                                                                double *__restrict__ loss_acc) {
    const int gid = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) / G);
    const int lg = threadIdx.x & (G - 1);
    const bool active = gid < cnt;
    const int64_t t = off + (active ? gid : cnt - 1);
    const int64_t j = lpos ? (int64_t)lpos[t] : t;
    const int32_t u = uid[j], i = cid[j];
    const float r = val[j];
    const float *pu = U + (size_t)u * k, *pi = V + (size_t)i * k;
    const float bu = Bu[u], bi = Bi[i];
    float pred = mu + bu + bi;
    for (int base = 0; base < k; base += G) {
        const int f = base + lg;
        float p = 0.f;
        if (f < k) p = pu[f] * pi[f];
        pred = ordered_lane_sum<G>(pred, p, min(G, k - base));
    }
    const float err = r - pred;
    double e2 = 0.0;
    if (active && lg == 0) {
        pred_out[j] = pred;
        if (use_bias) {
            Bu[u] = bu + lr * (err - lbu * bu);
            Bi[i] = bi + lr * (err - lbi * bi);
        }
        e2 = (double)(err * err);
    }
    const double l = wave_sum_f64(e2);
    if (lane_id() == 0 && l != 0.0) atomicAdd(loss_acc, l);
}

struct NmfChainArgs {
    ChainArgs c;   // rows = users, csid / cseq / cr = the CSR's items, positions inside the item, ratings: a position IS the stored index j
    const float *U, *V;
    float *Bu, *Bi, *pred;
    double *loss_acc;
    int k;
    float lr, lbu, lbi, mu;
};

// 64 / G ready ratings per pass, one per lane group (as pmf_det_chain_kernel), users owned
template <int G>
__global__ __launch_bounds__(kBlock) void nmf_bias_chain_kernel(const NmfChainArgs a) {
    const int k = a.k;
    double err2 = 0.0;
    chain_run<G>(a.c, [&](const ChainPass p) {
        const int32_t u = p.oid, i = p.sid;
        const float *pu = a.U + (size_t)u * k, *pi = a.V + (size_t)i * k;
        const float bu = p.act ? a.Bu[u] : 0.f, bi = p.act ? load_f32_sys(a.Bi + i) : 0.f;
        // ---- the reference's expression tree (nmf_bias_level_kernel) ----
        float pred = a.mu + bu + bi;
        for (int fb = 0; fb < k; fb += G) {
            const int f = fb + p.lg;
            float x = 0.f;
            if (p.act && f < k) x = pu[f] * pi[f];
            pred = ordered_lane_sum<G>(pred, x, min(G, k - fb));
        }
        const float err = p.r - pred;
        if (p.act && p.lg == 0) {
            a.pred[p.pos] = pred;
            a.Bu[u] = bu + a.lr * (err - a.lbu * bu);
            store_f32_sys(a.Bi + i, bi + a.lr * (err - a.lbi * bi));
            err2 += (double)(err * err);
        }
    });
    const double l = wave_sum_f64(err2);
    if (lane_id() == 0 && l != 0.0) atomicAdd(a.loss_acc, l);
}

}  // namespace chip

// ---- host: plans, kernel choice, epochs --------------------------------------------------------------------------------
typedef void (*NmfSumKernel)(const NmfSumArgs);
typedef void (*NmfChainKernel)(const NmfChainArgs);

static int nmf_group(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : kWave; }

template <bool ORDERED, bool PRED>
static NmfSumKernel pick_nmf_sum_kernel_t(int k) {
    if (k <= 8) return nmf_sum_kernel<8, 1, ORDERED, PRED>;
    if (k <= 16) return nmf_sum_kernel<16, 1, ORDERED, PRED>;
    if (k <= 32) return nmf_sum_kernel<32, 1, ORDERED, PRED>;
    if (k <= 64) return nmf_sum_kernel<64, 1, ORDERED, PRED>;
    if (k <= 128) return nmf_sum_kernel<64, 2, ORDERED, PRED>;
    if (k <= 192) return nmf_sum_kernel<64, 3, ORDERED, PRED>;
    return nmf_sum_kernel<64, 4, ORDERED, PRED>;
}

static NmfSumKernel pick_nmf_sum_kernel(int k, bool ordered, bool pred) {
    if (k > kNmfFastK) return nmf_sum_generic_kernel;
    if (ordered) return pred ? pick_nmf_sum_kernel_t<true, true>(k) : pick_nmf_sum_kernel_t<true, false>(k);
    return pred ? pick_nmf_sum_kernel_t<false, true>(k) : pick_nmf_sum_kernel_t<false, false>(k);
}

static NmfChainKernel pick_nmf_chain_kernel(int k) {
    switch (nmf_group(k)) {
        case 8: return nmf_bias_chain_kernel<8>;
        case 16: return nmf_bias_chain_kernel<16>;
        case 32: return nmf_bias_chain_kernel<32>;
        default: return nmf_bias_chain_kernel<64>;
    }
}

template <class T>
static void nmf_put(DevBuf<T> &b, const std::vector<T> &v, hipStream_t s) {
    b.alloc(std::max<size_t>(v.size(), 1));
    if (!v.empty()) b.upload(v.data(), v.size(), s);
}

// the CSR / CSC views of the stored order, once per handle.  The reference always walks the CSR of train_set.matrix
// (recom_nmf.pyx:168-178): a handle whose ratings are not stored by user is refused.
static void nmf_build(cornac_hip_mf_t h) {
    if (h->nmf_built) return;
    const int64_t n = h->nnz, nu = h->n_users, ni = h->n_items;
    REQUIRE(n < (int64_t(1) << 31), "NMF: more than 2^31 - 1 ratings");
    for (int64_t s = 1; s < n; ++s)
        REQUIRE(h->host_rid[(size_t)s] >= h->host_rid[(size_t)s - 1],
                "NMF needs the ratings stored by user (rid non-decreasing: the CSR of the rating matrix); rating %lld breaks the order",
                (long long)s);
    std::vector<int64_t> uptr((size_t)nu + 1, 0), iptr((size_t)ni + 1, 0);
    std::vector<int32_t> uid((size_t)n), cid((size_t)n), perm((size_t)n), cuid((size_t)n), cseq((size_t)n);
    for (int64_t s = 0; s < n; ++s) {
        uid[(size_t)s] = (int32_t)h->host_rid[(size_t)s];
        cid[(size_t)s] = (int32_t)h->host_cid[(size_t)s];
        ++uptr[(size_t)uid[(size_t)s] + 1];
        ++iptr[(size_t)cid[(size_t)s] + 1];
    }
    for (int64_t u = 0; u < nu; ++u) uptr[(size_t)u + 1] += uptr[(size_t)u];
    for (int64_t i = 0; i < ni; ++i) iptr[(size_t)i + 1] += iptr[(size_t)i];
    std::vector<int64_t> cur(iptr.begin(), iptr.end() - 1);
    for (int64_t s = 0; s < n; ++s) {   // stable: ascending stored position inside an item
        const int32_t i = cid[(size_t)s];
        const int64_t p = cur[(size_t)i]++;
        perm[(size_t)p] = (int32_t)s;
        cuid[(size_t)p] = uid[(size_t)s];
        cseq[(size_t)s] = (int32_t)(p - iptr[(size_t)i]);
    }
    h->nmf_uptr_h = uptr;
    h->nmf_iptr_h = iptr;
    nmf_put(h->nmf_uptr, uptr, h->stream); nmf_put(h->nmf_iptr, iptr, h->stream);
    nmf_put(h->nmf_uid, uid, h->stream); nmf_put(h->nmf_cid, cid, h->stream);
    nmf_put(h->nmf_perm, perm, h->stream); nmf_put(h->nmf_cuid, cuid, h->stream); nmf_put(h->nmf_cseq, cseq, h->stream);
    h->nmf_pred.alloc((size_t)n);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->nmf_built = true;
}

// segments of one side: whole rows (split == 0) or pieces of at most `split` ratings; longest first, so that the lane
// groups of a wave carry like loads and the long rows start early.  Every row has a segment (an empty one writes zeros).
static void nmf_build_segments(cornac_hip_mf_t h, NmfSide &sd, const std::vector<int64_t> &ptr, int split, int32_t slot0,
                               int32_t *n_slots) {
    const int64_t rows = (int64_t)ptr.size() - 1;
    std::vector<int32_t> row, len, dst, c_row, c_slot, c_n;
    std::vector<int64_t> beg;
    int32_t slot = slot0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t b = ptr[(size_t)r], cnt = ptr[(size_t)r + 1] - b;
        if (split <= 0 || cnt <= split) {
            REQUIRE(cnt < (int64_t(1) << 31), "NMF: a row of more than 2^31 - 1 ratings");
            row.push_back((int32_t)r); beg.push_back(b); len.push_back((int32_t)cnt); dst.push_back((int32_t)r);
            continue;
        }
        const int32_t pieces = (int32_t)((cnt + split - 1) / split);
        c_row.push_back((int32_t)r); c_slot.push_back(slot); c_n.push_back(pieces);
        for (int32_t q = 0; q < pieces; ++q) {
            row.push_back((int32_t)r); beg.push_back(b + (int64_t)q * split);
            len.push_back((int32_t)std::min<int64_t>(split, cnt - (int64_t)q * split));
            dst.push_back(-(slot++) - 1);
        }
    }
    std::vector<int32_t> order(row.size());
    for (size_t x = 0; x < order.size(); ++x) order[x] = (int32_t)x;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return len[(size_t)x] > len[(size_t)y]; });
    std::vector<int32_t> row2(row.size()), len2(row.size()), dst2(row.size());
    std::vector<int64_t> beg2(row.size());
    for (size_t x = 0; x < order.size(); ++x) {
        row2[x] = row[(size_t)order[x]]; len2[x] = len[(size_t)order[x]]; dst2[x] = dst[(size_t)order[x]]; beg2[x] = beg[(size_t)order[x]];
    }
    nmf_put(sd.seg_row, row2, h->stream); nmf_put(sd.seg_len, len2, h->stream); nmf_put(sd.seg_dst, dst2, h->stream);
    nmf_put(sd.seg_beg, beg2, h->stream);
    nmf_put(sd.c_row, c_row, h->stream); nmf_put(sd.c_slot, c_slot, h->stream); nmf_put(sd.c_n, c_n, h->stream);
    sd.n_seg = (int64_t)row2.size();
    sd.n_comb = (int64_t)c_row.size();
    *n_slots = slot;
}

// plans[0]: deterministic (whole rows), plans[1]: hogwild (long rows split)
static void nmf_build_plan(cornac_hip_mf_t h, int mode) {
    NmfPlan &pl = h->nmf_plan[mode];
    if (pl.built) return;
    const int split = mode == CORNAC_HIP_MODE_HOGWILD ? kNmfSplit : 0;
    int32_t slots = 0;
    nmf_build_segments(h, pl.side[0], h->nmf_uptr_h, split, 0, &slots);
    nmf_build_segments(h, pl.side[1], h->nmf_iptr_h, split, slots, &slots);
    pl.part.alloc(std::max<size_t>((size_t)slots * 2 * h->k, 1));
    pl.n_slots = slots;
    pl.rows_split = (int)(pl.side[0].n_comb + pl.side[1].n_comb);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    pl.built = true;
}

// the dataflow plan of the bias pass: users onto waves (chain_deal; a wave's users in CSR order), their CSR ranges as the
// rows' ratings.  Returns false where the occupancy query admits fewer than two workgroups per CU.
static bool nmf_build_chain(cornac_hip_mf_t h) {
    if (h->nmf_chain_built) return h->nmf_chain.grid > 0;
    h->nmf_chain_built = true;
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pick_nmf_chain_kernel(h->k), kBlock, 0));
    if (per_cu < 2) return false;   // half of an answer of 1 would be the whole admitted grid: the level schedule instead
    // half of what the query admits (mf_build_chain: every block of the grid stays resident)
    const int grid = device_info(h->device).cus * (std::min(per_cu, 8) / 2);
    const std::vector<int64_t> &uptr = h->nmf_uptr_h;
    std::vector<int64_t> cnt((size_t)h->n_users), wrow_ptr;
    for (int64_t u = 0; u < h->n_users; ++u) cnt[(size_t)u] = uptr[(size_t)u + 1] - uptr[(size_t)u];
    std::vector<int32_t> row_id;
    chain_deal(cnt, uptr, (int64_t)grid * kWavesPerBlock, wrow_ptr, row_id);
    std::vector<int64_t> row_beg(row_id.size()), row_end(row_id.size());
    for (size_t q = 0; q < row_id.size(); ++q) {
        row_beg[q] = uptr[(size_t)row_id[q]];
        row_end[q] = uptr[(size_t)row_id[q] + 1];
    }
    chain_upload(h->nmf_chain, grid, wrow_ptr, row_id, row_beg, row_end, h->n_items, h->stream);
    return true;
}

struct NmfHyper {
    float lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu;
};

// false when the runtime refuses the cooperative launch (nothing has run)
static bool nmf_bias_chain(cornac_hip_mf_t h, const NmfHyper &hy, double *loss_slot) {
    NmfChainArgs a;
    a.c = chain_args(h->nmf_chain, h->nmf_cid.p, h->nmf_cseq.p, h->val.p);
    a.U = h->nmf_U.p; a.V = h->nmf_V.p; a.Bu = h->nmf_Bu.p; a.Bi = h->nmf_Bi.p; a.pred = h->nmf_pred.p; a.loss_acc = loss_slot;
    a.k = h->k; a.lr = hy.lr; a.lbu = hy.lambda_bu; a.lbi = hy.lambda_bi; a.mu = hy.mu;
    return chain_launch(h->stream, h->nmf_chain, pick_nmf_chain_kernel(h->k), &a, "NMF bias dataflow kernel");
}

static void nmf_launch_level(cornac_hip_mf_t h, const int32_t *lpos, int64_t off, int cnt, const NmfHyper &hy, int use_bias,
                             double *loss_slot) {
    const int G = nmf_group(h->k);
    const int per_block = kBlock / G;
    const dim3 grid((unsigned int)(((int64_t)cnt + per_block - 1) / per_block)), block(kBlock);
#define NMF_LEVEL(GG)                                                                                                             \
    hipLaunchKernelGGL(nmf_bias_level_kernel<GG>, grid, block, 0, h->stream, lpos, h->nmf_uid.p, h->nmf_cid.p, h->val.p, off, cnt, \
                       h->nmf_U.p, h->nmf_V.p, h->nmf_Bu.p, h->nmf_Bi.p, h->nmf_pred.p, h->k, hy.lr, hy.lambda_bu, hy.lambda_bi,    \
                       hy.mu, use_bias, loss_slot)
    switch (G) {
        case 8: NMF_LEVEL(8); break;
        case 16: NMF_LEVEL(16); break;
        case 32: NMF_LEVEL(32); break;
        default: NMF_LEVEL(64); break;
    }
#undef NMF_LEVEL
}

// the level schedule of the stored order (mf_build_schedule's level_ptr) with the stored index of every schedule position
static void nmf_build_levels(cornac_hip_mf_t h) {
    if (h->nmf_levels_built) return;
    mf_build_schedule(h);
    const int64_t n = h->nnz;
    std::vector<int32_t> lvl_u((size_t)h->n_users, 0), lvl_i((size_t)h->n_items, 0), level((size_t)n), lpos((size_t)n);
    for (int64_t s = 0; s < n; ++s) {   // the recurrence of mf_build_schedule
        const size_t u = (size_t)h->host_rid[(size_t)s], i = (size_t)h->host_cid[(size_t)s];
        const int32_t l = std::max(lvl_u[u], lvl_i[i]) + 1;
        lvl_u[u] = lvl_i[i] = level[(size_t)s] = l;
    }
    // the positions are scattered through mf_build_schedule's level_ptr: hold this copy of the recurrence to it first
    const std::vector<int64_t> &lp = h->sched.level_ptr;
    std::vector<int64_t> count(lp.size(), 0);
    for (int64_t s = 0; s < n; ++s) {
        REQUIRE(level[(size_t)s] >= 1 && (size_t)level[(size_t)s] + 1 < lp.size(), "NMF: level schedules disagree (internal error)");
        ++count[(size_t)level[(size_t)s]];
    }
    for (size_t l = 1; l + 1 < lp.size(); ++l)
        REQUIRE(count[l] == lp[l + 1] - lp[l], "NMF: level schedules disagree at level %lld (internal error)", (long long)l);
    std::vector<int64_t> cursor(lp.begin(), lp.end());
    for (int64_t s = 0; s < n; ++s) lpos[(size_t)cursor[(size_t)level[(size_t)s]]++] = (int32_t)s;
    nmf_put(h->nmf_lpos, lpos, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->nmf_levels_built = true;
}

static void nmf_bias_levels(cornac_hip_mf_t h, const NmfHyper &hy, double *loss_slot) {
    nmf_build_levels(h);
    const std::vector<int64_t> &lp = h->sched.level_ptr;
    for (size_t l = 1; l + 1 < lp.size(); ++l) {
        const int cnt = (int)(lp[l + 1] - lp[l]);
        if (cnt > 0) nmf_launch_level(h, h->nmf_lpos.p, lp[l], cnt, hy, 1, loss_slot);
    }
    HIP_CHECK(hipGetLastError());
}

static void nmf_launch_sums(cornac_hip_mf_t h, NmfPlan &pl, int side, bool ordered, bool pred, const NmfHyper &hy, double *loss_slot) {
    NmfSide &sd = pl.side[side];
    NmfSumArgs a;
    a.seg_row = sd.seg_row.p; a.seg_len = sd.seg_len.p; a.seg_dst = sd.seg_dst.p; a.seg_beg = sd.seg_beg.p; a.n_seg = sd.n_seg;
    a.idx = side == 0 ? h->nmf_cid.p : h->nmf_cuid.p;
    a.pos = side == 0 ? nullptr : h->nmf_perm.p;
    a.val = h->val.p; a.pred = h->nmf_pred.p;
    a.own = side == 0 ? h->nmf_U.p : h->nmf_V.p; a.other = side == 0 ? h->nmf_V.p : h->nmf_U.p;
    a.b_own = side == 0 ? h->nmf_Bu.p : h->nmf_Bi.p; a.b_other = side == 0 ? h->nmf_Bi.p : h->nmf_Bu.p;
    a.mu = hy.mu;
    a.acc_num = side == 0 ? h->nmf_unum.p : h->nmf_vnum.p; a.acc_den = side == 0 ? h->nmf_uden.p : h->nmf_vden.p;
    a.part = pl.part.p; a.loss_acc = loss_slot; a.k = h->k;
    const int G = h->k > kNmfFastK ? kWave : nmf_group(h->k);
    const int per_block = kBlock / G;
    const int64_t grid = (sd.n_seg + per_block - 1) / per_block;
    hipLaunchKernelGGL(pick_nmf_sum_kernel(h->k, ordered, pred), dim3((unsigned int)grid), dim3(kBlock), 0, h->stream, a);
    if (sd.n_comb > 0)
        hipLaunchKernelGGL(nmf_combine_kernel, dim3((unsigned int)((sd.n_comb * h->k + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           h->stream, sd.c_row.p, sd.c_slot.p, sd.c_n.p, sd.n_comb, pl.part.p, a.acc_num, a.acc_den, h->k);
}

extern "C" {

int cornac_hip_mf_nmf_set_factors(cornac_hip_mf_t h, const float *U, const float *V, const float *Bu, const float *Bi) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(U && V, "U and V are required");
        const size_t nu = (size_t)h->n_users * h->k, ni = (size_t)h->n_items * h->k;
        h->nmf_U.ensure(nu); h->nmf_unum.ensure(nu); h->nmf_uden.ensure(nu);
        h->nmf_V.ensure(ni); h->nmf_vnum.ensure(ni); h->nmf_vden.ensure(ni);
        h->nmf_Bu.ensure((size_t)h->n_users); h->nmf_Bi.ensure((size_t)h->n_items);
        h->nmf_U.upload(U, nu, h->stream);
        h->nmf_V.upload(V, ni, h->stream);
        if (Bu) h->nmf_Bu.upload(Bu, (size_t)h->n_users, h->stream);
        else HIP_CHECK(hipMemsetAsync(h->nmf_Bu.p, 0, (size_t)h->n_users * sizeof(float), h->stream));
        if (Bi) h->nmf_Bi.upload(Bi, (size_t)h->n_items, h->stream);
        else HIP_CHECK(hipMemsetAsync(h->nmf_Bi.p, 0, (size_t)h->n_items * sizeof(float), h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->nmf_set = true;
    });
}

int cornac_hip_mf_nmf_get_factors(cornac_hip_mf_t h, float *U, float *V, float *Bu, float *Bi) {
    return guarded([&] {
        mf_check(h);
        REQUIRE(h->nmf_set, "cornac_hip_mf_nmf_set_factors has not been called on this handle");
        if (U) h->nmf_U.download(U, (size_t)h->n_users * h->k, h->stream);
        if (V) h->nmf_V.download(V, (size_t)h->n_items * h->k, h->stream);
        if (Bu) h->nmf_Bu.download(Bu, (size_t)h->n_users, h->stream);
        if (Bi) h->nmf_Bi.download(Bi, (size_t)h->n_items, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_mf_nmf_fit(cornac_hip_mf_t h, int n_epochs, float lr, float lambda_u, float lambda_v, float lambda_bu,
                          float lambda_bi, float mu, int use_bias, int mode, double *loss_per_epoch) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        REQUIRE(h->nmf_set, "cornac_hip_mf_nmf_fit before cornac_hip_mf_nmf_set_factors");
        REQUIRE(mode == CORNAC_HIP_MODE_DETERMINISTIC || mode == CORNAC_HIP_MODE_HOGWILD, "unknown mode %d", mode);
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        mf_check(h);
        nmf_build(h);
        nmf_build_plan(h, mode);
        NmfPlan &pl = h->nmf_plan[mode];
        const NmfHyper hy = {lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu};
        const bool ordered = mode == CORNAC_HIP_MODE_DETERMINISTIC, fast = h->k <= kNmfFastK;
        h->nmf_loss.ensure((size_t)std::max(n_epochs, 1));
        HIP_CHECK(hipMemsetAsync(h->nmf_loss.p, 0, h->nmf_loss.n * sizeof(double), h->stream));
        bool chain = use_bias && h->nnz >= 4096 && !h->nmf_chain_refused && !prof_env_set("CORNAC_HIP_MF_LEVELS");
        if (chain) chain = nmf_build_chain(h);
        const int n_all = (int)h->nnz;
        for (int e = 0; e < n_epochs; ++e) {
            double *slot = h->nmf_loss.p + e;
            int bias_form = 0;
            if (use_bias) {
                if (chain && nmf_bias_chain(h, hy, slot)) {
                    bias_form = 1;
                } else {
                    if (chain) {   // the dataflow launch was refused before anything ran: the level schedule from now on
                        chain = false;
                        h->nmf_chain_refused = true;
                    }
                    nmf_bias_levels(h, hy, slot);
                    bias_form = 2;
                }
            } else if (!fast) {
                nmf_launch_level(h, nullptr, 0, n_all, hy, 0, slot);   // r_pred alone, every rating independent
            }
            const bool pred = !use_bias && fast;
            nmf_launch_sums(h, pl, 0, ordered, pred, hy, slot);
            nmf_launch_sums(h, pl, 1, ordered, false, hy, slot);
            const int64_t eu = h->n_users * h->k, ei = h->n_items * h->k;
            hipLaunchKernelGGL(nmf_update_kernel, dim3((unsigned int)((eu + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                               h->nmf_U.p, h->nmf_unum.p, h->nmf_uden.p, h->nmf_uptr.p, h->n_users, h->k, lambda_u, slot);
            hipLaunchKernelGGL(nmf_update_kernel, dim3((unsigned int)((ei + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                               h->nmf_V.p, h->nmf_vnum.p, h->nmf_vden.p, h->nmf_iptr.p, h->n_items, h->k, lambda_v, slot);
            HIP_CHECK(hipGetLastError());
            h->nmf_sum_form = ordered ? 1 : 2;
            h->nmf_bias_form = bias_form;
            h->nmf_rows_split = pl.rows_split;
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (loss_per_epoch && n_epochs > 0)
            HIP_CHECK(hipMemcpy(loss_per_epoch, h->nmf_loss.p, sizeof(double) * (size_t)n_epochs, hipMemcpyDeviceToHost));
    });
}

int cornac_hip_mf_nmf_form(cornac_hip_mf_t h, int *sum_form, int *bias_form, int *rows_split) {
    return guarded([&] {
        REQUIRE(h != nullptr, "MF handle is NULL");
        if (sum_form) *sum_form = h->nmf_sum_form;
        if (bias_form) *bias_form = h->nmf_bias_form;
        if (rows_split) *rows_split = h->nmf_rows_split;
    });
}
}

// BiVAECF (Truong, Salah, Lauw 2021; cornac/models/bivaecf/bivae.py:34-276, recom_bivaecf.py:193-225) on gfx950, float32
// throughout: two one-hidden-layer encoders over the binary rows of X (users) and of X^T (items), each decoded by a bilinear
// product against the other side's sampled factor table, which is a constant of the step.  One handle owns the binarised
// CSR and its CSC, the 12 tables with Adam's moments, two step counters, and theta, beta, mu_theta, mu_beta.
//
// Every kernel takes "rows of this side, table of the other side": the item pass runs them over the CSC against theta, the
// user pass over the CSR against beta.  A step, for rows r0 .. r0 + B of the side (stream order):
//   encode    one workgroup per row: a1 as a sum of W1 rows over the row's entries in ascending order (no dense X, empty
//             rows included), h1, mu, s = sigmoid(.), z = mu + eps s, KL
//   dense     the fused decode: logits of the B rows against a fixed range of T's rows, tile by tile through LDS, sigmoid,
//             the log-likelihood and dL/do of an entry with x = 0, and dL/do . T accumulated in registers; writes
//             [S x B x k] and [S x B] partials, never a B x N array
//   backward  one workgroup per row: the partials summed in ascending range order, then the row's held entries in ascending
//             order, each adding f(1, p) - f(0, p) (all three likelihoods are affine in a binary x); then back through
//             z, s = sigmoid, mu and the KL terms to ga1
//   small Adam, W1 Adam   as vaecf.hip: one thread per entry; W1's is vae_device.h's kernel, which finds the batch's holders
//             of a column by bisection in the other orientation's index list; columns nobody of the batch holds get g = 0
//             and still decay and move
//   encode    again with the updated tables and the second noise plane: z and mu go to the side's factor tables
// No float atomics; every sum has one fixed order, so the same inputs give the same bits.
//
// The dense pass is register-tiled vector FMA (64 x 64 logit tiles, 4 x 4 per thread; then 64 x 16 gradient tiles, 4 per
// thread and 16-column chunk): f32-input MFMA has vector FMA's peak on this part, and the chains stay ascending this way.
#include "rng.h"
#include "vae_host.h"

namespace chip {
namespace {

constexpr int kBvMaxK = 256, kBvMaxH = 1024, kBvMaxBatch = 1024;
constexpr int kBvTile = 64, kBvTk = 16;
constexpr int kBvRange = CORNAC_HIP_BIVAE_RANGE;   // rows of T per workgroup of the dense pass
constexpr float kBvEps = 1e-10f;
constexpr int64_t kBvScoreBytes = 256ll << 20;   // a scoring chunk's rows
enum { LIK_BERN = 0, LIK_GAUS, LIK_POIS, LIK_COUNT };
enum { SIDE_USER = 0, SIDE_ITEM = 1 };
static_assert(kBvRange % kBvTile == 0, "a range is whole tiles");

// offsets (floats) of a side's six tables in its parameter buffer (W1 one row per id of the OTHER side); m and v alike
struct BvLayout {
    int64_t W1, b1, Wm, bm, Ws, bs, total;
};

// an entry with x = 0: its log-likelihood and -dLL/dp (bivae.py:136-140)
template <int LIK>
__device__ inline float bv_ll_absent(float p) {
    return LIK == LIK_BERN ? logf(1.f - p + kBvEps) : LIK == LIK_GAUS ? -(p * p) : -p;
}
template <int LIK>
__device__ inline float bv_g_absent(float p) {
    return LIK == LIK_BERN ? 1.f / (1.f - p + kBvEps) : LIK == LIK_GAUS ? 2.f * p : 1.f;
}

// what x = 1 adds to both
__device__ inline float bv_ll_held(int lik, float p) {
    const float d = 1.f - p;
    return lik == LIK_BERN ? logf(p + kBvEps) - logf(d + kBvEps) : lik == LIK_GAUS ? p * p - d * d : logf(p + kBvEps);
}
__device__ inline float bv_g_held(int lik, float p) {
    return lik == LIK_BERN ? -1.f / (p + kBvEps) - 1.f / (1.f - p + kBvEps) : lik == LIK_GAUS ? -2.f : -1.f / (p + kBvEps);
}

// ---- noise: eps[draw, row, c] of one side for a whole epoch, keyed by (seed, side, step of the row's batch, draw, row, factor) ----
__global__ void bv_noise_kernel(float *eps, int64_t n, int k, int64_t batch_size, int64_t t0, int side, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n * k) return;
    const int64_t draw = e / (n * k), r = (e % (n * k)) / k, c = e % k, t = t0 + r / batch_size + 1;
    uint32_t o[4];
    philox4x32_10((uint32_t)r, (uint32_t)c, (uint32_t)t, ((uint32_t)((uint64_t)t >> 32) << 2) | ((uint32_t)draw << 1) | (uint32_t)side,
                  (uint32_t)seed, (uint32_t)(seed >> 32), o);
    eps[e] = normal(o[0], o[1]);
}

// ---- encode: one workgroup per row (bivae.py:103-109, 119-121) --------------------------------------------------------------------
// The batch buffers (h1 .. kl) may be NULL together (the forward after the step, infer_means); z_out / mu_out are the
// side's factor tables, row = id, and may be NULL.  eps == NULL: z = mu.
__global__ __launch_bounds__(kVaeBlock) void bv_encode_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, int64_t r0, const float *__restrict__ w, BvLayout L, int h,
    int k, int act, const float *__restrict__ eps, float *h1, float *d1, float *mu, float *sd, float *z, float *kl, float *z_out,
    float *mu_out) {
    __shared__ float s_h[kBvMaxH];
    __shared__ float s_t[kBvMaxK];
    const int64_t b = blockIdx.x, r = r0 + b;
    const int64_t lo = row_ptr[r], hi = row_ptr[r + 1];
    const float *W1 = w + L.W1;
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        float a = 0.f;
        for (int64_t e = lo; e < hi; ++e) a += W1[(int64_t)row_idx[e] * h + j];
        a += w[L.b1 + j];
        float d;
        const float v = vae_act(act, a, &d);
        if (h1) {
            h1[b * h + j] = v;
            d1[b * h + j] = d;
        }
        s_h[j] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kVaeBlock) {
        const float *wm = w + L.Wm + (int64_t)c * h, *ws = w + L.Ws + (int64_t)c * h;
        float m = 0.f, a = 0.f;
        for (int j = 0; j < h; ++j) {
            m = fmaf(s_h[j], wm[j], m);
            a = fmaf(s_h[j], ws[j], a);
        }
        m += w[L.bm + c];
        a += w[L.bs + c];
        const float s = 1.f / (1.f + expf(-a));
        const float zz = eps ? m + eps[r * k + c] * s : m;
        if (mu) {
            mu[b * k + c] = m;
            sd[b * k + c] = s;
            z[b * k + c] = zz;
        }
        if (z_out) z_out[r * k + c] = zz;
        if (mu_out) mu_out[r * k + c] = m;
        s_t[c] = 1.f + 2.f * logf(s) - m * m - s * s;
    }
    __syncthreads();
    if (threadIdx.x == 0 && kl) {
        float acc = 0.f;
        for (int c = 0; c < k; ++c) acc += s_t[c];
        kl[b] = -0.5f * acc;
    }
}

// ---- the fused decode, dense pass: every entry as x = 0 ------------------------------------------------------------------------------
// Workgroup (s, y): the batch rows [64 y, 64 y + 64) against T's rows [s kBvRange, (s + 1) kBvRange), 64 at a time:
//   o = Z T^T (chains over the factors, ascending), p = sigmoid(o), ll += LL(0, p), g = dL/do / B into LDS,
//   acc2[b, c] += sum_n g[b, n] T[n, c]  (n ascending, over the whole range)
// and at the end part_g[s, b, c] = acc2, part_ll[s, b] = ll (the row's 16 thread sums in ascending order).  k <= 16 KC.
template <int KC, int LIK>
__global__ __launch_bounds__(kVaeBlock) void bv_dense_kernel(const float *__restrict__ Z, const float *__restrict__ T, int64_t N, int k,
                                                             int64_t nb, float inv_b, float *part_g, float *part_ll) {
    __shared__ float sZ[kBvTk][kBvTile + 4];
    __shared__ float sT[kBvTk][kBvTile + 4];
    __shared__ float sG[kBvTile][kBvTile + 4];   // [n][b]
    __shared__ float sC[kBvTile][kBvTk + 1];     // [n][c]: 16 columns of the tile's rows of T
    const int64_t s = blockIdx.x, b0 = (int64_t)blockIdx.y * kBvTile;
    const int64_t n_begin = s * kBvRange, n_end = N < n_begin + kBvRange ? N : n_begin + kBvRange;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    float acc2[KC][4], ll[4];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc2[kc][p] = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) ll[p] = 0.f;
    for (int64_t n0 = n_begin; n0 < n_end; n0 += kBvTile) {
        float acc[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = 0.f;
        for (int c0 = 0; c0 < k; c0 += kBvTk) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = threadIdx.x + kVaeBlock * q;
                const int cc = idx % kBvTk, mm = idx / kBvTk;
                const int64_t gb = b0 + mm, gn = n0 + mm;
                const int gc = c0 + cc;
                sZ[cc][mm] = (gb < nb && gc < k) ? Z[gb * k + gc] : 0.f;
                sT[cc][mm] = (gn < n_end && gc < k) ? T[gn * k + gc] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int cc = 0; cc < kBvTk; ++cc) {
                float a[4], t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = sZ[cc][ty * 4 + q];
                    t[q] = sT[cc][tx * 4 + q];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(a[p], t[q], acc[p][q]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float g = 0.f;
                if (b0 + ty * 4 + p < nb && n0 + tx * 4 + q < n_end) {
                    const float pr = 1.f / (1.f + expf(-acc[p][q]));
                    ll[p] += bv_ll_absent<LIK>(pr);
                    g = bv_g_absent<LIK>(pr) * pr * (1.f - pr) * inv_b;
                }
                sG[tx * 4 + q][ty * 4 + p] = g;
            }
        __syncthreads();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            if (kc * kBvTk >= k) break;   // (the same for every thread)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = threadIdx.x + kVaeBlock * q;
                const int cc = idx % kBvTk, nn = idx / kBvTk;
                const int64_t gn = n0 + nn;
                const int gc = kc * kBvTk + cc;
                sC[nn][cc] = (gn < n_end && gc < k) ? T[gn * k + gc] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int nn = 0; nn < kBvTile; ++nn) {
                const float t = sC[nn][tx];
#pragma unroll
                for (int p = 0; p < 4; ++p) acc2[kc][p] = fmaf(sG[nn][ty * 4 + p], t, acc2[kc][p]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int64_t gb = b0 + ty * 4 + p;
            const int c = kc * kBvTk + tx;
            if (gb < nb && c < k) part_g[(s * nb + gb) * k + c] = acc2[kc][p];
        }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) sG[ty * 4 + p][tx] = ll[p];
    __syncthreads();
    if (threadIdx.x < kBvTile && b0 + threadIdx.x < nb) {
        float acc = 0.f;
        for (int x = 0; x < 16; ++x) acc += sG[threadIdx.x][x];
        part_ll[s * nb + b0 + threadIdx.x] = acc;
    }
}

// ---- backward: one workgroup per row ------------------------------------------------------------------------------------------------
// gz and LL from the dense partials (ascending range order), the correction over the row's held entries (ascending, 256 at
// a time: their logits side by side, then each factor's chain), loss[r] = beta KL - LL (bivae.py:134-152), and the chain
// back through z = mu + eps s, s = sigmoid(a_s), mu and the KL terms to ga1.
__global__ __launch_bounds__(kVaeBlock) void bv_backward_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, int64_t r0, const float *__restrict__ Z,
    const float *__restrict__ T, const float *__restrict__ part_g, const float *__restrict__ part_ll, int64_t n_split, int64_t nb,
    const float *__restrict__ w, BvLayout L, int h, int k, int lik, float beta, float inv_b, const float *__restrict__ eps,
    const float *__restrict__ d1, const float *__restrict__ mu, const float *__restrict__ sd, const float *__restrict__ kl, float *gmu,
    float *gas, float *ga1, float *loss) {
    __shared__ float s_dg[kVaeBlock];
    __shared__ float s_dl[kVaeBlock];
    __shared__ int32_t s_n[kVaeBlock];
    __shared__ float s_z[kBvMaxK];
    __shared__ float s_m[kBvMaxK];
    __shared__ float s_v[kBvMaxK];
    const int64_t b = blockIdx.x, r = r0 + b;
    const int64_t lo = row_ptr[r], hi = row_ptr[r + 1];
    const int c = threadIdx.x;   // (k <= 256: one thread per factor)
    float gz = 0.f, ll = 0.f;
    if (c < k) {
        s_z[c] = Z[b * k + c];
        for (int64_t s = 0; s < n_split; ++s) gz += part_g[(s * nb + b) * k + c];
    }
    if (c == 0)
        for (int64_t s = 0; s < n_split; ++s) ll += part_ll[s * nb + b];
    __syncthreads();
    for (int64_t e0 = lo; e0 < hi; e0 += kVaeBlock) {
        const int64_t e = e0 + threadIdx.x;
        if (e < hi) {
            const int32_t n = row_idx[e];
            const float *t = T + (int64_t)n * k;
            float o = 0.f;
            for (int q = 0; q < k; ++q) o = fmaf(s_z[q], t[q], o);
            const float pr = 1.f / (1.f + expf(-o));
            s_dg[threadIdx.x] = bv_g_held(lik, pr) * pr * (1.f - pr) * inv_b;
            s_dl[threadIdx.x] = bv_ll_held(lik, pr);
            s_n[threadIdx.x] = n;
        }
        __syncthreads();
        const int cnt = (int)(hi - e0 < kVaeBlock ? hi - e0 : kVaeBlock);
        if (c < k)
            for (int j = 0; j < cnt; ++j) gz = fmaf(s_dg[j], T[(int64_t)s_n[j] * k + c], gz);
        if (c == 0)
            for (int j = 0; j < cnt; ++j) ll += s_dl[j];
        __syncthreads();
    }
    if (c < k) {
        const float m = mu[b * k + c], s = sd[b * k + c];
        const float gm = gz + beta * m * inv_b;
        const float gs = gz * eps[r * k + c] + beta * (s - 1.f / s) * inv_b;
        const float ga = gs * s * (1.f - s);
        gmu[b * k + c] = gm;
        gas[b * k + c] = ga;
        s_m[c] = gm;
        s_v[c] = ga;
    }
    if (c == 0) loss[r] = beta * kl[b] - ll;
    __syncthreads();
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        const float *wm = w + L.Wm, *ws = w + L.Ws;
        float g = 0.f;
        for (int q = 0; q < k; ++q) {
            g = fmaf(s_m[q], wm[(int64_t)q * h + j], g);
            g = fmaf(s_v[q], ws[(int64_t)q * h + j], g);
        }
        ga1[b * h + j] = g * d1[b * h + j];
    }
}

// ---- Adam on the small tables: Wm bm Ws bs b1, one thread per entry ---------------------------------------------------------------
__global__ void bv_small_adam_kernel(float *w, float *am, float *av, BvLayout L, int h, int k, int64_t nb, const float *__restrict__ gmu,
                                     const float *__restrict__ gas, const float *__restrict__ h1, const float *__restrict__ ga1,
                                     VaeAdam ad) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hk = (int64_t)h * k;
    const float *x = nullptr, *y = nullptr;   // g = sum_b x[b, xi] * y[b, yi]  (y == nullptr: sum_b x[b, xi])
    int64_t xs = 0, ys = 0, xi = 0, yi = 0, at = 0;
    if (e < hk) { x = gmu; xs = k; xi = e / h; y = h1; ys = h; yi = e % h; at = L.Wm + e; }
    else if ((e -= hk) < k) { x = gmu; xs = k; xi = e; at = L.bm + e; }
    else if ((e -= k) < hk) { x = gas; xs = k; xi = e / h; y = h1; ys = h; yi = e % h; at = L.Ws + e; }
    else if ((e -= hk) < k) { x = gas; xs = k; xi = e; at = L.bs + e; }
    else if ((e -= k) < h) { x = ga1; xs = h; xi = e; at = L.b1 + e; }
    else return;
    float g = 0.f;
    if (y) for (int64_t b = 0; b < nb; ++b) g = fmaf(x[b * xs + xi], y[b * ys + yi], g);
    else for (int64_t b = 0; b < nb; ++b) g += x[b * xs + xi];
    vae_adam(w, am, av, at, g, ad);
}

// ---- scores: sigmoid(<mu_theta[u], mu_beta[i]>), one thread per entry; items == NULL: the rows of users[0 .. nb) --------------------
__global__ void bv_score_kernel(const float *__restrict__ mu_theta, const float *__restrict__ mu_beta, const int32_t *__restrict__ users,
                                const int32_t *__restrict__ items, int64_t nb, int64_t I, int k, float *out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (items ? nb : nb * I)) return;
    const int64_t u = users[items ? e : e / I], i = items ? (int64_t)items[e] : e % I;
    const float *a = mu_theta + u * k, *t = mu_beta + i * k;
    float o = 0.f;
    for (int q = 0; q < k; ++q) o = fmaf(a[q], t[q], o);
    out[e] = 1.f / (1.f + expf(-o));
}

struct BvSide {
    int64_t n = 0, N = 0;   // this side's ids; the other side's (W1's input width, and the decoder's table length)
    int64_t t = 0;          // this side's Adam step counter
    BvLayout L{};
    std::vector<TableSlot> slots;   // this side's six tables of w / m / v in the reference's state_dict order
    const DevCsr *own = nullptr, *other = nullptr;   // this side's rows; the other orientation
    DevBuf<float> w, m, v, z, mu, eps, loss;         // z: theta or beta [n x k]; mu: mu_theta or mu_beta
};

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_bivae : ModelHandle {
    int64_t n_users = 0, n_items = 0;
    int k = 0, h = 0, act = 0, lik = 0;
    DevCsr rows, cols;   // the binarised X and its transpose: no values
    BvSide side[2];      // SIDE_USER, SIDE_ITEM
    // per call, sized for `cap` rows
    int64_t cap = 0;
    DevBuf<float> h1, d1, mu, sd, z, kl, gmu, gas, ga1, part_g, part_ll, out;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // the last epoch's start, end of the item pass, end of the user pass
    float pass_ms[2] = {0.f, 0.f};                    // SIDE_USER, SIDE_ITEM
    ~cornac_hip_bivae() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

static int64_t bv_splits(int64_t N) { return (N + kBvRange - 1) / kBvRange; }

static void bv_ensure(cornac_hip_bivae_t h, int64_t cap) {
    if (cap <= h->cap) return;
    const size_t hh = (size_t)h->h, k = (size_t)h->k, c = (size_t)cap;
    const size_t S = (size_t)bv_splits(std::max(h->n_users, h->n_items));
    const char *what = "a batch's activations and partial sums";
    for (DevBuf<float> *b : {&h->h1, &h->d1, &h->ga1}) alloc_named(*b, c * hh, "BiVAECF", what);
    for (DevBuf<float> *b : {&h->mu, &h->sd, &h->z, &h->gmu, &h->gas}) alloc_named(*b, c * k, "BiVAECF", what);
    alloc_named(h->kl, c, "BiVAECF", what);
    alloc_named(h->part_g, S * c * k, "BiVAECF", what);
    alloc_named(h->part_ll, S * c, "BiVAECF", what);
    h->cap = cap;
}

int cornac_hip_bivae_create(cornac_hip_bivae_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                            const int32_t *indices, int k, int hidden, int act, int likelihood) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "BiVAECF: sizes must be positive");
        REQUIRE(n_users < (1ll << 31) && n_items < (1ll << 31), "BiVAECF: user and item counts must fit int32");
        REQUIRE(k >= 1 && k <= kBvMaxK, "BiVAECF: k = %d is outside the supported range 1 <= k <= %d", k, kBvMaxK);
        REQUIRE(hidden >= 1 && hidden <= kBvMaxH, "BiVAECF: h = %d is outside the supported range 1 <= h <= %d", hidden, kBvMaxH);
        REQUIRE(act >= 0 && act < ACT_COUNT, "BiVAECF: unknown activation %d", act);
        REQUIRE(likelihood >= 0 && likelihood < LIK_COUNT, "BiVAECF: unknown likelihood %d", likelihood);
        check_csr("BiVAECF", "X", n_users, n_items, indptr, indices, nullptr, kCsrNoValues);
        const HostCsr t = transpose_csr(n_users, n_items, indptr, indices, nullptr);   // the items' users, ascending
        std::unique_ptr<cornac_hip_bivae> h(new cornac_hip_bivae());
        h->open(device);
        h->n_users = n_users; h->n_items = n_items;
        h->k = k; h->h = hidden; h->act = act; h->lik = likelihood;
        h->rows.upload("BiVAECF", "X", n_users, indptr, indices, nullptr, h->stream);
        h->cols.upload("BiVAECF", "X transposed", t, h->stream);
        for (int s = 0; s < 2; ++s) {
            BvSide &d = h->side[s];
            d.n = s == SIDE_USER ? n_users : n_items;
            d.N = s == SIDE_USER ? n_items : n_users;
            d.own = s == SIDE_USER ? &h->rows : &h->cols;
            d.other = s == SIDE_USER ? &h->cols : &h->rows;
            const int64_t hh = hidden, kk = k;
            BvLayout &L = d.L;
            L.W1 = 0; L.b1 = L.W1 + d.N * hh; L.Wm = L.b1 + hh; L.bm = L.Wm + kk * hh; L.Ws = L.bm + kk; L.bs = L.Ws + kk * hh;
            L.total = L.bs + kk;
            // in the reference's shapes: fc0.weight is [h x N] there, [N x h] here
            d.slots = {{L.W1, hh, d.N, true}, {L.b1, 1, hh, false}, {L.Wm, kk, hh, false},
                       {L.bm, 1, kk, false}, {L.Ws, kk, hh, false}, {L.bs, 1, kk, false}};
            for (DevBuf<float> *b : {&d.w, &d.m, &d.v}) alloc_named(*b, (size_t)L.total, "BiVAECF", "the tables and Adam's moments");
            for (DevBuf<float> *b : {&d.z, &d.mu}) alloc_named(*b, (size_t)(d.n * kk), "BiVAECF", "the factor tables");
            alloc_named(d.eps, (size_t)(2 * d.n * kk), "BiVAECF", "the noise");
            alloc_named(d.loss, (size_t)d.n, "BiVAECF", "the rows' losses");
            for (DevBuf<float> *b : {&d.w, &d.m, &d.v, &d.z, &d.mu}) HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        for (hipEvent_t &e : h->ev) HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_bivae_destroy(cornac_hip_bivae_t h) { return destroy_handle(h); }

// host <-> device copies of the 12 tables of one kind (the buffer `buf` of a side): the user side's six, then the item side's
static void bv_put(cornac_hip_bivae_t h, DevBuf<float> BvSide::*buf, const float *const *tables) {
    for (int s = 0; s < 2; ++s) put_tables(h->stream, (h->side[s].*buf).p, h->side[s].slots, tables + 6 * s);
}

static void bv_get(cornac_hip_bivae_t h, DevBuf<float> BvSide::*buf, float *const *tables) {
    for (int s = 0; s < 2; ++s) get_tables(h->stream, (h->side[s].*buf).p, h->side[s].slots, tables + 6 * s);
}

int cornac_hip_bivae_set_params(cornac_hip_bivae_t h, const float *const *tables) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        REQUIRE(tables != nullptr, "BiVAECF: tables is NULL");
        bv_put(h, &BvSide::w, tables);
    });
}

int cornac_hip_bivae_get_params(cornac_hip_bivae_t h, float *const *tables) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        REQUIRE(tables != nullptr, "BiVAECF: tables is NULL");
        bv_get(h, &BvSide::w, tables);
    });
}

int cornac_hip_bivae_set_factors(cornac_hip_bivae_t h, const float *theta, const float *beta, const float *mu_theta, const float *mu_beta) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        BvSide &u = h->side[SIDE_USER], &i = h->side[SIDE_ITEM];
        if (theta) u.z.upload(theta, u.z.n, h->stream);
        if (beta) i.z.upload(beta, i.z.n, h->stream);
        if (mu_theta) u.mu.upload(mu_theta, u.mu.n, h->stream);
        if (mu_beta) i.mu.upload(mu_beta, i.mu.n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_bivae_get_factors(cornac_hip_bivae_t h, float *theta, float *beta, float *mu_theta, float *mu_beta) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        const BvSide &u = h->side[SIDE_USER], &i = h->side[SIDE_ITEM];
        if (theta) u.z.download(theta, u.z.n, h->stream);
        if (beta) i.z.download(beta, i.z.n, h->stream);
        if (mu_theta) u.mu.download(mu_theta, u.mu.n, h->stream);
        if (mu_beta) i.mu.download(mu_beta, i.mu.n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_bivae_get_state(cornac_hip_bivae_t h, float *const *m, float *const *v, int64_t *t_user, int64_t *t_item) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        if (m) bv_get(h, &BvSide::m, m);
        if (v) bv_get(h, &BvSide::v, v);
        if (t_user) *t_user = h->side[SIDE_USER].t;
        if (t_item) *t_item = h->side[SIDE_ITEM].t;
    });
}

int cornac_hip_bivae_reset_optimizer(cornac_hip_bivae_t h) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        BvSide &u = h->side[SIDE_USER], &i = h->side[SIDE_ITEM];
        zero_state(h->stream, {&u.m, &u.v, &i.m, &i.v});
        u.t = i.t = 0;
    });
}

// the dense pass of nb rows in h->z against T [N x k]
static void bv_dense(cornac_hip_bivae_t h, const float *T, int64_t N, int64_t nb, float inv_b) {
    const dim3 grid((unsigned)bv_splits(N), (unsigned)((nb + kBvTile - 1) / kBvTile));
    const int kc = (h->k + kBvTk - 1) / kBvTk;
#define BV_DENSE_L(KC, LIK) \
    bv_dense_kernel<KC, LIK><<<grid, kVaeBlock, 0, h->stream>>>(h->z.p, T, N, h->k, nb, inv_b, h->part_g.p, h->part_ll.p)
#define BV_DENSE(KC) \
    do { \
        if (h->lik == LIK_BERN) BV_DENSE_L(KC, LIK_BERN); \
        else if (h->lik == LIK_GAUS) BV_DENSE_L(KC, LIK_GAUS); \
        else BV_DENSE_L(KC, LIK_POIS); \
    } while (0)
    if (kc <= 1) BV_DENSE(1);
    else if (kc <= 2) BV_DENSE(2);
    else if (kc <= 4) BV_DENSE(4);
    else if (kc <= 8) BV_DENSE(8);
    else BV_DENSE(16);
#undef BV_DENSE
#undef BV_DENSE_L
}

// one side's pass of an epoch (bivae.py:198-223 for the items, :228-252 for the users): the steps' kernels, enqueued
static void bv_side_epoch(cornac_hip_bivae_t h, int s, int64_t batch_size, float lr, float beta) {
    BvSide &d = h->side[s];
    const BvSide &o = h->side[1 - s];
    const int hh = h->h, k = h->k;
    const int64_t small = 2 * (int64_t)hh * k + 2 * k + hh;
    float *w = d.w.p, *am = d.m.p, *av = d.v.p;
    const float *eps1 = d.eps.p, *eps2 = d.eps.p + d.n * k;
    for (int64_t r0 = 0; r0 < d.n; r0 += batch_size) {
        const int64_t nb = std::min(batch_size, d.n - r0);
        const float inv_b = 1.0f / (float)nb;
        d.t += 1;
        const VaeAdam ad = adam_at(d.t, lr);
        bv_encode_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(d.own->ptr.p, d.own->idx.p, r0, w, d.L, hh, k, h->act, eps1, h->h1.p,
                                                                   h->d1.p, h->mu.p, h->sd.p, h->z.p, h->kl.p, nullptr, nullptr);
        bv_dense(h, o.z.p, d.N, nb, inv_b);
        bv_backward_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(d.own->ptr.p, d.own->idx.p, r0, h->z.p, o.z.p, h->part_g.p,
                                                                     h->part_ll.p, bv_splits(d.N), nb, w, d.L, hh, k, h->lik, beta, inv_b,
                                                                     eps1, h->d1.p, h->mu.p, h->sd.p, h->kl.p, h->gmu.p, h->gas.p,
                                                                     h->ga1.p, d.loss.p);
        bv_small_adam_kernel<<<grid(small), kVaeBlock, 0, h->stream>>>(w, am, av, d.L, hh, k, nb, h->gmu.p, h->gas.p, h->h1.p, h->ga1.p, ad);
        vae_w1_adam_kernel<<<grid(d.N * hh), kVaeBlock, 0, h->stream>>>(w, am, av, d.L.W1, d.N, hh, r0, nb, d.other->ptr.p, d.other->idx.p,
                                                                        h->ga1.p, ad);
        // bivae.py:220-223 / 250-252: the forward again, with the updated tables and fresh noise, into the factor tables
        bv_encode_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(d.own->ptr.p, d.own->idx.p, r0, w, d.L, hh, k, h->act, eps2, nullptr,
                                                                   nullptr, nullptr, nullptr, nullptr, nullptr, d.z.p, d.mu.p);
        HIP_CHECK(hipGetLastError());
    }
}

int cornac_hip_bivae_fit_epoch(cornac_hip_bivae_t h, int64_t batch_size, float lr, float beta_kl, const float *eps_item,
                               const float *eps_user, uint64_t seed, double *loss_item, double *loss_user, double *step_loss) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        REQUIRE(batch_size >= 1 && batch_size <= kBvMaxBatch, "BiVAECF: batch_size = %lld is outside the supported range 1 <= batch_size <= %d",
                (long long)batch_size, kBvMaxBatch);
        REQUIRE(std::isfinite(lr) && std::isfinite(beta_kl), "BiVAECF: lr and beta_kl must be finite");
        bv_ensure(h, std::min(batch_size, std::max(h->n_users, h->n_items)));
        HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
        for (int s : {SIDE_ITEM, SIDE_USER}) {
            BvSide &d = h->side[s];
            const float *eps = s == SIDE_ITEM ? eps_item : eps_user;
            if (eps) d.eps.upload(eps, d.eps.n, h->stream);
            else bv_noise_kernel<<<grid(2 * d.n * h->k), kVaeBlock, 0, h->stream>>>(d.eps.p, d.n, h->k, batch_size, d.t, s, seed);
            bv_side_epoch(h, s, batch_size, lr, beta_kl);
            HIP_CHECK(hipEventRecord(h->ev[s == SIDE_ITEM ? 1 : 2], h->stream));
        }
        std::vector<float> loss[2];
        for (int s = 0; s < 2; ++s) {
            loss[s].resize((size_t)h->side[s].n);
            h->side[s].loss.download(loss[s].data(), loss[s].size(), h->stream);
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipEventElapsedTime(&h->pass_ms[SIDE_ITEM], h->ev[0], h->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&h->pass_ms[SIDE_USER], h->ev[1], h->ev[2]));
        int64_t step = 0;
        for (int s : {SIDE_ITEM, SIDE_USER}) {
            const int64_t n = h->side[s].n;
            double total = 0.0;
            for (int64_t r0 = 0; r0 < n; r0 += batch_size, ++step) {
                const int64_t nb = std::min(batch_size, n - r0);
                double acc = 0.0;
                for (int64_t b = 0; b < nb; ++b) acc += (double)loss[s][(size_t)(r0 + b)];
                acc /= (double)nb;
                if (step_loss) step_loss[step] = acc;
                total += acc;
            }
            double *dst = s == SIDE_ITEM ? loss_item : loss_user;
            if (dst) *dst = total;
        }
    });
}

int cornac_hip_bivae_last_timing(cornac_hip_bivae_t h, double *item_ms, double *user_ms) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        if (item_ms) *item_ms = h->pass_ms[SIDE_ITEM];
        if (user_ms) *user_ms = h->pass_ms[SIDE_USER];
    });
}

int cornac_hip_bivae_infer_means(cornac_hip_bivae_t h) {
    return guarded([&] {
        check_handle(h, "BiVAECF handle");
        for (int s : {SIDE_ITEM, SIDE_USER}) {
            BvSide &d = h->side[s];
            for (int64_t r0 = 0; r0 < d.n; r0 += kBvMaxBatch) {
                const int64_t nb = std::min<int64_t>(kBvMaxBatch, d.n - r0);
                bv_encode_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(d.own->ptr.p, d.own->idx.p, r0, d.w.p, d.L, h->h, h->k, h->act,
                                                                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                           nullptr, d.mu.p);
            }
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

// users[0 .. n) in chunks: the rows (items == NULL) or the pairs' entries
static void bv_predict(cornac_hip_bivae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    check_handle(h, "BiVAECF handle");
    check_ids("BiVAECF", users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t I = h->n_items;
    const int64_t B = std::min<int64_t>(n, std::max<int64_t>(1, std::min<int64_t>(kBvMaxBatch, kBvScoreBytes / (4 * I))));
    const size_t need = (size_t)(items ? B : B * I);
    if (h->out.n < need) alloc_named(h->out, need, "BiVAECF", "the scores");
    for_each_chunk("BiVAECF", *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        const int64_t cnt = items ? nb : nb * I;
        bv_score_kernel<<<grid(cnt), kVaeBlock, 0, h->stream>>>(h->side[SIDE_USER].mu.p, h->side[SIDE_ITEM].mu.p, h->user_ids.p,
                                                                items ? h->item_ids.p : nullptr, nb, I, h->k, h->out.p);
        h->out.download(out + (items ? b0 : b0 * I), (size_t)cnt, h->stream);
    });
}

int cornac_hip_bivae_score_users(cornac_hip_bivae_t h, const int32_t *users, int64_t n, float *out) {
    return guarded([&] { bv_predict(h, users, nullptr, n, out); });
}

int cornac_hip_bivae_score_pairs(cornac_hip_bivae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "BiVAECF: items is NULL");
        bv_predict(h, users, items, n, out);
    });
}

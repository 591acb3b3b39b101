// VAECF (Liang et al. 2018; cornac/models/vaecf/vaecf.py:37-149, recom_vaecf.py:167-202) on gfx950, float32 throughout:
// the minibatch forward and backward of a one-hidden-layer variational autoencoder over binary rows, torch.optim.Adam's
// dense sweep over all ten tables, and the scores decode(mu(x_u)).  One handle owns the binarised training CSR and its
// CSC, the tables with Adam's moments (one buffer each: W1 stored one row per item), and the step counter.
//
// A step, for users u0 .. u0 + B of the batch (stream order):
//   encode     one workgroup per user: a1 as a sum of W1 rows over the row's items in ascending order (no dense X),
//              h1, mu, logvar, std, z = mu + eps std, KL, a2, h2
//   logits     o = h2 D1^T + c1                       [B x I]   tiled FMA
//   likelihood one workgroup per user: p, the log-likelihood, dL/do in place of o (the row maximum is subtracted)
//   gh2        go D1, split over fixed item ranges    [S x B x h] tiled FMA, summed in ascending range order by
//   middle     one workgroup per user: ga2, gz, gmu, glv, ga1
//   small Adam one thread per entry of D0 c0 Wm bm Wv bv b1: its gradient over the batch in ascending order, then Adam
//   W1 Adam    one thread per entry of W1: the gradient over the batch's users that hold the item (a range of the item's
//              ascending user list, found by bisection: batches are consecutive user ranges), then Adam; rows of absent
//              items get g = 0 and still decay and move
//   c1 Adam    one thread per item
//   D1 Adam    go^T h2 tile by tile, each tile applied to D1, m, v at once: no I x h gradient table
// No float atomics; every sum has one fixed order (thread-owned chains in ascending index, fixed trees in a workgroup),
// so the same inputs give the same bits.  Offsets into the I x h tables are 64-bit.
//
// The three B x h x I products are vae_device.h's register-tiled vector FMA (64 x 64 tiles, 4 x 4 per thread, operands staged
// through LDS), launched by vae_host.h's linear, linear_back_split and weight_adam: f32-input MFMA has vector FMA's peak on
// this part, and the chains keep a fixed ascending order this way.
#include "rng.h"
#include "vae_host.h"

namespace chip {
namespace {

constexpr int kVaeMaxK = 256, kVaeMaxH = 1024, kVaeMaxBatch = 1024;
constexpr float kVaeEps = 1e-10f;
constexpr int64_t kVaeScoreBytes = 256ll << 20;   // a scoring chunk's logits (at most kVaeMaxBatch users)
enum { LIK_MULT = 0, LIK_BERN, LIK_GAUS, LIK_POIS, LIK_COUNT };

// offsets (floats) of the ten tables in the parameter buffer; m and v use the same layout
struct VaeLayout {
    int64_t W1, b1, Wm, bm, Wv, bv, D0, c0, D1, c1, total;
};

__device__ inline bool vae_holds(const int32_t *__restrict__ idx, int64_t lo, int64_t hi, int32_t i) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < i) lo = mid + 1; else hi = mid;
    }
    return lo < end && idx[lo] == i;
}

// ---- noise: eps[u, c] for a whole epoch, keyed by (seed, step of the user's batch, user, factor) ----------------------------
__global__ void vae_noise_kernel(float *eps, int64_t n_users, int k, int64_t batch_size, int64_t t0, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_users * k) return;
    const int64_t u = e / k, c = e % k, t = t0 + u / batch_size + 1;
    uint32_t r[4];
    philox4x32_10((uint32_t)u, (uint32_t)c, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    eps[e] = normal(r[0], r[1]);
}

// ---- encode: one workgroup per user ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVaeBlock) void vae_encode_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, const int32_t *__restrict__ users, int64_t u0,
    const float *__restrict__ w, VaeLayout L, int h, int k, int act, const float *__restrict__ eps, float *h1, float *d1, float *mu,
    float *sd, float *z, float *h2, float *d2, float *kl) {
    __shared__ float s_h[kVaeMaxH];
    __shared__ float s_z[kVaeMaxK];
    __shared__ float s_t[kVaeMaxK];
    const int64_t b = blockIdx.x, u = users ? (int64_t)users[b] : u0 + b;
    const int64_t lo = row_ptr[u], hi = row_ptr[u + 1];
    const float *W1 = w + L.W1;
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        float a = 0.f;
        for (int64_t e = lo; e < hi; ++e) a += W1[(int64_t)row_idx[e] * h + j];
        a += w[L.b1 + j];
        float d;
        const float v = vae_act(act, a, &d);
        h1[b * h + j] = v;
        d1[b * h + j] = d;
        s_h[j] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kVaeBlock) {
        const float *wm = w + L.Wm + (int64_t)c * h, *wv = w + L.Wv + (int64_t)c * h;
        float m = 0.f, lv = 0.f;
        for (int j = 0; j < h; ++j) {
            m = fmaf(s_h[j], wm[j], m);
            lv = fmaf(s_h[j], wv[j], lv);
        }
        m += w[L.bm + c];
        lv += w[L.bv + c];
        const float s = expf(0.5f * lv);
        const float zz = eps ? m + eps[u * k + c] * s : m;
        mu[b * k + c] = m;
        sd[b * k + c] = s;
        z[b * k + c] = zz;
        s_z[c] = zz;
        s_t[c] = 1.f + lv - m * m - s * s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int c = 0; c < k; ++c) acc += s_t[c];
        kl[b] = -0.5f * acc;
    }
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        const float *d0 = w + L.D0 + (int64_t)j * k;
        float a = 0.f;
        for (int c = 0; c < k; ++c) a = fmaf(s_z[c], d0[c], a);
        a += w[L.c0 + j];
        float d;
        h2[b * h + j] = vae_act(act, a, &d);
        d2[b * h + j] = d;
    }
}

// ---- likelihood: one workgroup per row of the logits --------------------------------------------------------------------------
// train != 0: row <- dL/do (divided by the batch's size), loss[u] = beta KL - LL.  train == 0: row <- p.
__global__ __launch_bounds__(kVaeBlock) void vae_likelihood_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, const int32_t *__restrict__ users, int64_t u0,
    float *o, int64_t I, int lik, int train, float inv_b, float beta, const float *__restrict__ kl, float *loss) {
    __shared__ float sh[kVaeBlock];
    const int64_t b = blockIdx.x, u = users ? (int64_t)users[b] : u0 + b;
    const int64_t lo = row_ptr[u], hi = row_ptr[u + 1];
    float *row = o + b * I;
    float ll = 0.f;
    if (lik == LIK_MULT) {
        float mx = -INFINITY;
        for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) mx = fmaxf(mx, row[i]);
        mx = block_max(mx, sh);
        float se = 0.f;
        for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) {
            const float e = expf(row[i] - mx);
            row[i] = e;
            se += e;
        }
        se = block_sum(se, sh);   // (its barriers also order the stores of e before the reads below)
        for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) row[i] = row[i] / se;
        __syncthreads();
        if (!train) return;
        float s = 0.f;
        for (int64_t e = lo + threadIdx.x; e < hi; e += kVaeBlock) {
            const float p = row[row_idx[e]];
            ll += logf(p + kVaeEps);
            s += -p / (p + kVaeEps);
        }
        s = block_sum(s, sh);
        ll = block_sum(ll, sh);
        for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) {
            const float p = row[i];
            const float g = vae_holds(row_idx, lo, hi, (int32_t)i) ? -1.f / (p + kVaeEps) : 0.f;
            row[i] = p * (g - s) * inv_b;
        }
    } else {
        for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) {
            const float p = 1.f / (1.f + expf(-row[i]));
            if (!train) { row[i] = p; continue; }
            const bool x = vae_holds(row_idx, lo, hi, (int32_t)i);
            float g;
            if (lik == LIK_BERN) {
                ll += x ? logf(p + kVaeEps) : logf(1.f - p + kVaeEps);
                g = x ? -1.f / (p + kVaeEps) : 1.f / (1.f - p + kVaeEps);
            } else if (lik == LIK_GAUS) {
                const float d = (x ? 1.f : 0.f) - p;
                ll += -(d * d);
                g = -2.f * d;
            } else {
                ll += x ? logf(p + kVaeEps) - p : -p;
                g = x ? 1.f - 1.f / (p + kVaeEps) : 1.f;
            }
            row[i] = g * p * (1.f - p) * inv_b;
        }
        if (!train) return;
        ll = block_sum(ll, sh);
    }
    if (threadIdx.x == 0) loss[u] = beta * kl[b] - ll;
}

// ---- middle: one workgroup per user ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVaeBlock) void vae_middle_kernel(
    const float *__restrict__ part, int n_split, int64_t nb, int64_t u0, const float *__restrict__ w, VaeLayout L, int h, int k,
    float beta, float inv_b, const float *__restrict__ eps, const float *__restrict__ d1, const float *__restrict__ d2,
    const float *__restrict__ mu, const float *__restrict__ sd, float *ga2, float *gmu, float *glv, float *ga1) {
    __shared__ float s_a[kVaeMaxH];
    __shared__ float s_m[kVaeMaxK];
    __shared__ float s_v[kVaeMaxK];
    const int64_t b = blockIdx.x, u = u0 + b;
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        float g = 0.f;
        for (int s = 0; s < n_split; ++s) g += part[((int64_t)s * nb + b) * h + j];
        g *= d2[b * h + j];
        ga2[b * h + j] = g;
        s_a[j] = g;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += kVaeBlock) {
        const float *d0 = w + L.D0;
        float gz = 0.f;
        for (int j = 0; j < h; ++j) gz = fmaf(s_a[j], d0[(int64_t)j * k + c], gz);
        const float m = mu[b * k + c], s = sd[b * k + c];
        const float gm = gz + beta * m * inv_b;
        const float gv = gz * eps[u * k + c] * s * 0.5f - beta * (1.f - s * s) * 0.5f * inv_b;
        gmu[b * k + c] = gm;
        glv[b * k + c] = gv;
        s_m[c] = gm;
        s_v[c] = gv;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        const float *wm = w + L.Wm, *wv = w + L.Wv;
        float g = 0.f;
        for (int c = 0; c < k; ++c) {
            g = fmaf(s_m[c], wm[(int64_t)c * h + j], g);
            g = fmaf(s_v[c], wv[(int64_t)c * h + j], g);
        }
        ga1[b * h + j] = g * d1[b * h + j];
    }
}

// ---- Adam on the small tables: D0 c0 Wm bm Wv bv b1, one thread per entry ---------------------------------------------------------
__global__ void vae_small_adam_kernel(float *w, float *am, float *av, VaeLayout L, int h, int k, int64_t nb,
                                      const float *__restrict__ ga2, const float *__restrict__ z, const float *__restrict__ gmu,
                                      const float *__restrict__ glv, const float *__restrict__ h1, const float *__restrict__ ga1,
                                      VaeAdam ad) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t hk = (int64_t)h * k;
    const float *x = nullptr, *y = nullptr;   // g = sum_b x[b, xi] * y[b, yi]  (y == nullptr: sum_b x[b, xi])
    int64_t xs = 0, ys = 0, xi = 0, yi = 0, at = 0;
    if (e < hk) { x = ga2; xs = h; xi = e / k; y = z; ys = k; yi = e % k; at = L.D0 + e; }
    else if ((e -= hk) < h) { x = ga2; xs = h; xi = e; at = L.c0 + e; }
    else if ((e -= h) < hk) { x = gmu; xs = k; xi = e / h; y = h1; ys = h; yi = e % h; at = L.Wm + e; }
    else if ((e -= hk) < k) { x = gmu; xs = k; xi = e; at = L.bm + e; }
    else if ((e -= k) < hk) { x = glv; xs = k; xi = e / h; y = h1; ys = h; yi = e % h; at = L.Wv + e; }
    else if ((e -= hk) < k) { x = glv; xs = k; xi = e; at = L.bv + e; }
    else if ((e -= k) < h) { x = ga1; xs = h; xi = e; at = L.b1 + e; }
    else return;
    float g = 0.f;
    if (y) for (int64_t b = 0; b < nb; ++b) g = fmaf(x[b * xs + xi], y[b * ys + yi], g);
    else for (int64_t b = 0; b < nb; ++b) g += x[b * xs + xi];
    vae_adam(w, am, av, at, g, ad);
}

__global__ void vae_c1_adam_kernel(float *w, float *am, float *av, VaeLayout L, int64_t I, int64_t nb, const float *__restrict__ go,
                                   VaeAdam ad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    float g = 0.f;
    for (int64_t b = 0; b < nb; ++b) g += go[b * I + i];
    vae_adam(w, am, av, L.c1 + i, g, ad);
}

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_vaecf : ModelHandle {
    int64_t n_users = 0, n_items = 0, nnz = 0;
    int k = 0, h = 0, act = 0, lik = 0;
    int64_t t = 0;   // Adam's step counter
    VaeLayout L{};
    std::vector<TableSlot> slots;   // the ten tables of w / m / v in the reference's state_dict order
    DevCsr rows, cols;   // the binarised X and its transpose: no values
    DevBuf<float> w, m, v, eps, loss;
    // per call, sized for `cap` rows
    int64_t cap = 0;
    int n_split = 1;
    int64_t kchunk = 0;
    DevBuf<float> h1, d1, mu, sd, z, h2, d2, kl, logits, part, ga2, gmu, glv, ga1, out;
};

static void vae_ensure(cornac_hip_vaecf_t h, int64_t cap) {
    if (cap <= h->cap) return;
    const size_t I = (size_t)h->n_items, hh = (size_t)h->h, k = (size_t)h->k, c = (size_t)cap;
    h->n_split = (int)std::min<int64_t>(32, std::max<int64_t>(1, (h->n_items + 4095) / 4096));
    h->kchunk = ((h->n_items + h->n_split - 1) / h->n_split + kVaeTk - 1) / kVaeTk * kVaeTk;
    const char *what = "a batch's activations and logits";
    for (DevBuf<float> *b : {&h->h1, &h->d1, &h->h2, &h->d2, &h->ga2, &h->ga1}) alloc_named(*b, c * hh, "VAECF", what);
    for (DevBuf<float> *b : {&h->mu, &h->sd, &h->z, &h->gmu, &h->glv}) alloc_named(*b, c * k, "VAECF", what);
    alloc_named(h->kl, c, "VAECF", what);
    alloc_named(h->logits, c * I, "VAECF", what);
    alloc_named(h->part, (size_t)h->n_split * c * hh, "VAECF", what);
    h->cap = cap;
}

int cornac_hip_vaecf_create(cornac_hip_vaecf_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                            const int32_t *indices, int k, int hidden, int act, int likelihood) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "VAECF: sizes must be positive");
        REQUIRE(n_users < (1ll << 31) && n_items < (1ll << 31), "VAECF: user and item counts must fit int32");
        REQUIRE(k >= 1 && k <= kVaeMaxK, "VAECF: k = %d is outside the supported range 1 <= k <= %d", k, kVaeMaxK);
        REQUIRE(hidden >= 1 && hidden <= kVaeMaxH, "VAECF: h = %d is outside the supported range 1 <= h <= %d", hidden, kVaeMaxH);
        REQUIRE(act >= 0 && act < ACT_COUNT, "VAECF: unknown activation %d", act);
        REQUIRE(likelihood >= 0 && likelihood < LIK_COUNT, "VAECF: unknown likelihood %d", likelihood);
        check_csr("VAECF", "X", n_users, n_items, indptr, indices, nullptr, kCsrNoValues);
        const HostCsr t = transpose_csr(n_users, n_items, indptr, indices, nullptr);   // the items' users, ascending
        std::unique_ptr<cornac_hip_vaecf> h(new cornac_hip_vaecf());
        h->open(device);
        h->n_users = n_users; h->n_items = n_items; h->nnz = indptr[n_users];
        h->k = k; h->h = hidden; h->act = act; h->lik = likelihood;
        {
            const int64_t I = n_items, hh = hidden, kk = k;
            VaeLayout &L = h->L;
            L.W1 = 0; L.b1 = L.W1 + I * hh; L.Wm = L.b1 + hh; L.bm = L.Wm + kk * hh; L.Wv = L.bm + kk; L.bv = L.Wv + kk * hh;
            L.D0 = L.bv + kk; L.c0 = L.D0 + hh * kk; L.D1 = L.c0 + hh; L.c1 = L.D1 + I * hh; L.total = L.c1 + I;
            // in the reference's shapes: W1 is [h x I] there, [I x h] here
            h->slots = {{L.W1, hh, I, true}, {L.b1, 1, hh, false}, {L.Wm, kk, hh, false}, {L.bm, 1, kk, false}, {L.Wv, kk, hh, false},
                        {L.bv, 1, kk, false}, {L.D0, hh, kk, false}, {L.c0, 1, hh, false}, {L.D1, I, hh, false}, {L.c1, 1, I, false}};
        }
        for (DevBuf<float> *b : {&h->w, &h->m, &h->v}) {
            alloc_named(*b, (size_t)h->L.total, "VAECF", "the tables and Adam's moments");
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        alloc_named(h->eps, (size_t)n_users * (size_t)k, "VAECF", "the noise");
        alloc_named(h->loss, (size_t)n_users, "VAECF", "the users' losses");
        h->rows.upload("VAECF", "X", n_users, indptr, indices, nullptr, h->stream);
        h->cols.upload("VAECF", "X transposed", t, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_vaecf_destroy(cornac_hip_vaecf_t h) { return destroy_handle(h); }

int cornac_hip_vaecf_set_params(cornac_hip_vaecf_t h, const float *const *tables) {
    return guarded([&] {
        check_handle(h, "VAECF handle");
        REQUIRE(tables != nullptr, "VAECF: tables is NULL");
        put_tables(h->stream, h->w.p, h->slots, tables);
    });
}

int cornac_hip_vaecf_get_params(cornac_hip_vaecf_t h, float *const *tables) {
    return guarded([&] {
        check_handle(h, "VAECF handle");
        REQUIRE(tables != nullptr, "VAECF: tables is NULL");
        get_tables(h->stream, h->w.p, h->slots, tables);
    });
}

int cornac_hip_vaecf_get_state(cornac_hip_vaecf_t h, float *const *m, float *const *v, int64_t *t) {
    return guarded([&] {
        check_handle(h, "VAECF handle");
        if (m) get_tables(h->stream, h->m.p, h->slots, m);
        if (v) get_tables(h->stream, h->v.p, h->slots, v);
        if (t) *t = h->t;
    });
}

int cornac_hip_vaecf_reset_optimizer(cornac_hip_vaecf_t h) {
    return guarded([&] {
        check_handle(h, "VAECF handle");
        zero_state(h->stream, {&h->m, &h->v});
        h->t = 0;
    });
}

// h2 of nb rows -> logits[nb x I]
static void vae_logits(cornac_hip_vaecf_t h, int64_t nb) {
    linear(h->stream, "VAECF", h->h2.p, h->w.p + h->L.D1, h->w.p + h->L.c1, nullptr, nb, h->n_items, h->h, h->logits.p);
}

int cornac_hip_vaecf_fit_epoch(cornac_hip_vaecf_t h, int64_t batch_size, float lr, float beta, const float *eps, uint64_t seed,
                               double *loss_sum, double *step_loss) {
    return guarded([&] {
        check_handle(h, "VAECF handle");
        REQUIRE(batch_size >= 1 && batch_size <= kVaeMaxBatch, "VAECF: batch_size = %lld is outside the supported range 1 <= batch_size <= %d",
                (long long)batch_size, kVaeMaxBatch);
        REQUIRE(std::isfinite(lr) && std::isfinite(beta), "VAECF: lr and beta must be finite");
        const int64_t nu = h->n_users, I = h->n_items, hh = h->h, k = h->k;
        vae_ensure(h, std::min(batch_size, nu));
        if (eps) h->eps.upload(eps, (size_t)(nu * k), h->stream);
        else vae_noise_kernel<<<grid(nu * k), kVaeBlock, 0, h->stream>>>(h->eps.p, nu, (int)k, batch_size, h->t, seed);
        float *w = h->w.p, *am = h->m.p, *av = h->v.p;
        const VaeLayout L = h->L;
        const int64_t small = 3 * hh * k + 2 * hh + 2 * k;
        const int64_t n_steps = (nu + batch_size - 1) / batch_size;
        for (int64_t s = 0; s < n_steps; ++s) {
            const int64_t u0 = s * batch_size, nb = std::min(batch_size, nu - u0);
            const float inv_b = 1.0f / (float)nb;
            h->t += 1;
            const VaeAdam ad = adam_at(h->t, lr);
            vae_encode_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, nullptr, u0, w, L, (int)hh, (int)k, h->act,
                                                                        h->eps.p, h->h1.p, h->d1.p, h->mu.p, h->sd.p, h->z.p, h->h2.p,
                                                                        h->d2.p, h->kl.p);
            vae_logits(h, nb);
            vae_likelihood_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, nullptr, u0, h->logits.p, I, h->lik, 1,
                                                                            inv_b, beta, h->kl.p, h->loss.p);
            // gh2 partials: go[nb x I] D1[I x h] over n_split item ranges
            linear_back_split(h->stream, "VAECF", h->logits.p, w + L.D1, nb, hh, I, h->kchunk, h->n_split, h->part.p);
            vae_middle_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->part.p, h->n_split, nb, u0, w, L, (int)hh, (int)k, beta, inv_b,
                                                                        h->eps.p, h->d1.p, h->d2.p, h->mu.p, h->sd.p, h->ga2.p, h->gmu.p,
                                                                        h->glv.p, h->ga1.p);
            vae_small_adam_kernel<<<grid(small), kVaeBlock, 0, h->stream>>>(w, am, av, L, (int)hh, (int)k, nb, h->ga2.p, h->z.p, h->gmu.p,
                                                                            h->glv.p, h->h1.p, h->ga1.p, ad);
            vae_w1_adam_kernel<<<grid(I * hh), kVaeBlock, 0, h->stream>>>(w, am, av, L.W1, I, (int)hh, u0, nb, h->cols.ptr.p, h->cols.idx.p,
                                                                          h->ga1.p, ad);
            vae_c1_adam_kernel<<<grid(I), kVaeBlock, 0, h->stream>>>(w, am, av, L, I, nb, h->logits.p, ad);
            // D1: (go^T h2)[I x h], each tile applied at once
            weight_adam(h->stream, "VAECF", h->logits.p, h->h2.p, nb, I, hh, w + L.D1, am + L.D1, av + L.D1, ad);
            HIP_CHECK(hipGetLastError());
        }
        std::vector<float> loss((size_t)nu);
        h->loss.download(loss.data(), (size_t)nu, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        double total = 0.0;
        for (int64_t s = 0; s < n_steps; ++s) {
            const int64_t u0 = s * batch_size, nb = std::min(batch_size, nu - u0);
            double acc = 0.0;
            for (int64_t b = 0; b < nb; ++b) acc += (double)loss[(size_t)(u0 + b)];
            acc /= (double)nb;
            if (step_loss) step_loss[s] = acc;
            total += acc;
        }
        if (loss_sum) *loss_sum = total;
    });
}

// users[0 .. n) in chunks: encode at z = mu; then h2 to the host (what == 0), p rows (1) or p[q, items[q]] (2)
static void vae_predict(cornac_hip_vaecf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out, int what) {
    check_handle(h, "VAECF handle");
    check_ids("VAECF", users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t I = h->n_items, hh = h->h;
    const int64_t B = std::min<int64_t>(n, std::max<int64_t>(1, std::min<int64_t>(kVaeMaxBatch, kVaeScoreBytes / (4 * I))));
    vae_ensure(h, B);
    if (items && h->out.n < (size_t)B) alloc_named(h->out, (size_t)B, "VAECF", "the scores");
    for_each_chunk("VAECF", *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        vae_encode_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, h->user_ids.p, 0, h->w.p, h->L, (int)hh, h->k,
                                                                    h->act, nullptr, h->h1.p, h->d1.p, h->mu.p, h->sd.p, h->z.p, h->h2.p,
                                                                    h->d2.p, h->kl.p);
        if (what == 0) {
            h->h2.download(out + b0 * hh, (size_t)(nb * hh), h->stream);
            return;
        }
        vae_logits(h, nb);
        vae_likelihood_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, h->user_ids.p, 0, h->logits.p, I, h->lik, 0,
                                                                        0.f, 0.f, h->kl.p, h->loss.p);
        if (what == 1) {
            h->logits.download(out + b0 * I, (size_t)(nb * I), h->stream);
        } else {
            gather_pairs_kernel<<<grid(nb), kVaeBlock, 0, h->stream>>>(h->logits.p, I, h->item_ids.p, nb, h->out.p);
            h->out.download(out + b0, (size_t)nb, h->stream);
        }
    });
}

int cornac_hip_vaecf_encode_users(cornac_hip_vaecf_t h, const int32_t *users, int64_t n, float *h2_out) {
    return guarded([&] { vae_predict(h, users, nullptr, n, h2_out, 0); });
}

int cornac_hip_vaecf_score_users(cornac_hip_vaecf_t h, const int32_t *users, int64_t n, float *out) {
    return guarded([&] { vae_predict(h, users, nullptr, n, out, 1); });
}

int cornac_hip_vaecf_score_pairs(cornac_hip_vaecf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "VAECF: items is NULL");
        vae_predict(h, users, items, n, out, 2);
    });
}

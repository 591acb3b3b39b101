// RecVAE (Shenbin et al. 2020; cornac/models/recvae/recvae.py:9-116, recom_recvae.py:127-146, 241-278) on gfx950, float32
// throughout: the minibatch forward and backward of a five-layer densely connected encoder (swish, LayerNorm eps 0.1) over
// L2-normalised rating rows under input dropout, a linear decoder, the KL term against the three-part composite prior, the
// two torch.optim.Adam sweeps (encoder's 24 tables, decoder's 2) and the scores decoder(mu(x_u)).  One handle owns the
// training CSR with its real values, the rows' norms and sums, the tables (fc1.weight stored one row per item), the frozen
// old encoder, the prior tables, Adam's moments and both step counters.
//
// A step, for the users order[s B .. s B + nb) (stream order):
//   input      one workgroup per user and 512 of its entries: the sum of x_e W1[item_e] over the kept ones, ascending; then
//              pre1 = the row's chunk sums in ascending order + b1 (the order depends on the row alone, not on the batch)
//   layer      one workgroup per user: h_l = LN_l(swish(pre_l)), keeping xhat_l; R <- h_1 + .. + h_l
//   dense      pre_{l+1} = h_l W_{l+1}^T + b_{l+1} + R;  mu, logvar = h_5 W^T + b            tiled FMA
//   latent     one workgroup per user: z = mu + eps exp(logvar / 2), the KL sum against the mixture (max-shifted)
//   logits     o = z D^T + c                                  [B x I], kept (the row's maximum and sum come before
//              its gradient, and B x I floats stay in the last-level cache at the shapes this model is run at)
//   likelihood one workgroup per user: sum_i x_i log_softmax(o)_i, dL/do in place of o
//   encoder    gz = go D over fixed item ranges, summed in ascending range order; the mixture's gradient in z, mu and
//   pass       logvar; back through LN, swish and the dense skip sums layer by layer; then Adam: the h x h and latent
//              tables tile by tile from gp^T h (no gradient table), the vectors one thread per entry over the batch in
//              ascending order, fc1 one thread per entry over the batch's users that hold the item with a kept entry
//   decoder    Adam on D from go^T z tile by tile and on c one thread per item
//   pass
// The old encoder's posterior is a function of the user alone between two update_prior calls: it is computed for every
// user once per update_prior with the forward kernels above and read per step.  Batches are arbitrary user ids, so each
// pass lists every item's entries in the pass's order (a counting sort on the host, one upload); a step's users are then a
// range of that list found by bisection, as in vae_device.h's vae_w1_adam_kernel.  No float atomics; every sum has one fixed
// order (thread-owned chains in ascending index, fixed trees in a workgroup): the same inputs give the same bits.  Offsets
// are 64-bit.
//
// The dense products are vae_device.h's register-tiled vector FMA (64 x 64 tiles, 4 x 4 per thread, operands staged through
// LDS), launched by vae_host.h's linear, linear_back, linear_back_split and weight_adam: f32-input MFMA has vector FMA's peak
// on this part, and the chains keep a fixed ascending order this way.
#include "rng.h"
#include "vae_host.h"

#include <memory>

namespace chip {
namespace {

constexpr int kRvMaxK = 256, kRvMaxH = 1024, kRvMaxBatch = 1024;
constexpr int kRvLayers = 5, kRvEncTables = 24, kRvTables = 53;
constexpr int kRvPerThread = kRvMaxH / kVaeBlock;
constexpr int kRvChunk = 512;   // entries of a row per workgroup of the input layer
constexpr float kRvLnEps = 0.1f, kRvLog2Pi = 1.8378770664093453f;
constexpr int64_t kRvScoreBytes = 256ll << 20;   // a scoring chunk's logits (at most kRvMaxBatch users)

// offsets (floats) of the encoder's tables in an encoder buffer, and of the decoder's behind them in the trainable buffer
struct RvLayout {
    int64_t W[kRvLayers], b[kRvLayers], g[kRvLayers], c[kRvLayers], Wm, bm, Wv, bv, enc_total, Wd, bd, total;
};

// ---- draws on the device: pure functions of (seed, pass key, entry) and (seed, pass key, user, column) ---------------------
__global__ void rv_keep_kernel(uint8_t *keep, int64_t nnz, float keep_share, uint64_t key, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    uint32_t r[4];
    philox4x32_10((uint32_t)e, (uint32_t)((uint64_t)e >> 32), (uint32_t)key, (uint32_t)(key >> 32) ^ 0x6b656570u, (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    keep[e] = unit(r[0]) < keep_share ? 1 : 0;
}

__global__ void rv_noise_kernel(float *eps, int64_t n_users, int k, uint64_t key, uint64_t seed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_users * k) return;
    uint32_t r[4];
    philox4x32_10((uint32_t)(e / k), (uint32_t)(e % k), (uint32_t)key, (uint32_t)(key >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    eps[e] = 0.01f * normal(r[0], r[1]);
}

// ---- input: one workgroup per user and chunk of kRvChunk of its entries ------------------------------------------------------
// part[b, c, j] = sum_e x_e W1[item_e, j] over the chunk's entries, ascending; x_e = xn[e] (times scale where keep[e], 0 where
// dropped).  The chunks depend on the row alone, so a user's sums have the same order in every batch.
__global__ __launch_bounds__(kVaeBlock) void rv_input_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx,
                                                             const float *__restrict__ xn, const uint8_t *__restrict__ keep, float scale,
                                                             const int32_t *__restrict__ users, const float *__restrict__ W1, int h,
                                                             float *part) {
    __shared__ int32_t s_idx[kRvChunk];
    __shared__ float s_x[kRvChunk];
    const int64_t b = blockIdx.x, c = blockIdx.y, u = users[b];
    const int64_t lo = row_ptr[u] + c * kRvChunk, end = row_ptr[u + 1];
    if (c > 0 && lo >= end) return;   // (chunk 0 of an empty row still writes its zeros)
    const int n = (int)(end - lo < kRvChunk ? (end > lo ? end - lo : 0) : kRvChunk);
    for (int t = threadIdx.x; t < n; t += kVaeBlock) {
        const int64_t e = lo + t;
        s_idx[t] = row_idx[e];
        s_x[t] = keep ? (keep[e] ? xn[e] * scale : 0.f) : xn[e];
    }
    __syncthreads();
    float *out = part + (b * gridDim.y + c) * h;
    for (int j = threadIdx.x; j < h; j += kVaeBlock) {
        float a = 0.f;
#pragma unroll 8
        for (int t = 0; t < n; ++t) a = fmaf(s_x[t], W1[(int64_t)s_idx[t] * h + j], a);
        out[j] = a;
    }
}

// pre[b, j] = the row's chunk sums in ascending chunk order, then + b1[j]
__global__ void rv_input_sum_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ users, const float *__restrict__ part,
                                    int n_chunks, const float *__restrict__ b1, int h, int64_t nb, float *pre) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nb * h) return;
    const int64_t b = e / h, j = e % h, u = users[b];
    const int64_t len = row_ptr[u + 1] - row_ptr[u];
    const int64_t nc = len > kRvChunk ? (len + kRvChunk - 1) / kRvChunk : 1;
    float a = 0.f;
    for (int64_t c = 0; c < nc; ++c) a += part[(b * n_chunks + c) * h + j];
    pre[e] = a + b1[j];
}

__device__ inline float rv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- layer: hid = LN(swish(pre)), one workgroup per row; R <- hid (first) or R + hid ---------------------------------------------
__global__ __launch_bounds__(kVaeBlock) void rv_layer_kernel(const float *__restrict__ pre, int h, const float *__restrict__ g,
                                                             const float *__restrict__ c, float *xhat, float *rstd, float *hid, float *R,
                                                             int first) {
    __shared__ float sh[kVaeBlock];
    const int64_t b = blockIdx.x;
    float s[kRvPerThread];
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < kRvPerThread; ++q) {
        const int j = threadIdx.x + q * kVaeBlock;
        s[q] = 0.f;
        if (j < h) {
            const float x = pre[b * h + j];
            s[q] = x * rv_sigmoid(x);
            acc += s[q];
        }
    }
    const float mean = block_sum(acc, sh) / (float)h;
    acc = 0.f;
#pragma unroll
    for (int q = 0; q < kRvPerThread; ++q) {
        const int j = threadIdx.x + q * kVaeBlock;
        if (j < h) {
            s[q] -= mean;
            acc += s[q] * s[q];
        }
    }
    const float r = 1.f / sqrtf(block_sum(acc, sh) / (float)h + kRvLnEps);
    if (threadIdx.x == 0) rstd[b] = r;
#pragma unroll
    for (int q = 0; q < kRvPerThread; ++q) {
        const int j = threadIdx.x + q * kVaeBlock;
        if (j < h) {
            const float xh = s[q] * r, y = xh * g[j] + c[j];
            xhat[b * h + j] = xh;
            hid[b * h + j] = y;
            R[b * h + j] = first ? y : R[b * h + j] + y;
        }
    }
}

// ---- layer backward: G = dL/dhid -> gp = dL/dpre, one workgroup per row; S <- gp (last layer) or S + gp --------------------------
__global__ __launch_bounds__(kVaeBlock) void rv_layer_back_kernel(const float *__restrict__ G, const float *__restrict__ pre,
                                                                  const float *__restrict__ xhat, const float *__restrict__ rstd, int h,
                                                                  const float *__restrict__ g, float *gp, float *S, int last) {
    __shared__ float sh[kVaeBlock];
    const int64_t b = blockIdx.x;
    float gx[kRvPerThread], xh[kRvPerThread];
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int q = 0; q < kRvPerThread; ++q) {
        const int j = threadIdx.x + q * kVaeBlock;
        gx[q] = xh[q] = 0.f;
        if (j < h) {
            gx[q] = G[b * h + j] * g[j];
            xh[q] = xhat[b * h + j];
            a1 += gx[q];
            a2 += gx[q] * xh[q];
        }
    }
    const float m1 = block_sum(a1, sh) / (float)h, m2 = block_sum(a2, sh) / (float)h, r = rstd[b];
#pragma unroll
    for (int q = 0; q < kRvPerThread; ++q) {
        const int j = threadIdx.x + q * kVaeBlock;
        if (j < h) {
            const float gs = r * (gx[q] - m1 - xh[q] * m2);
            const float x = pre[b * h + j], sg = rv_sigmoid(x);
            const float v = gs * (sg * (1.f + x * (1.f - sg)));
            gp[b * h + j] = v;
            S[b * h + j] = last ? v : S[b * h + j] + v;
        }
    }
}

// ---- the KL term of one latent column (recvae.py:12-13, 34-46, 106) ----------------------------------------------------------
struct RvKl {
    float term;    // log N(z; mu, logvar) - logsumexp_j(log w_j + log N(z; prior_j))
    float q_z;     // d log N(z; mu, logvar) / dz  (its derivative in mu is -q_z)
    float q_lv;    // d log N(z; mu, logvar) / dlogvar
    float p_z;     // d logsumexp / dz
};

__device__ inline float rv_log_norm(float x, float mu, float lv) {
    const float d = x - mu;
    return -0.5f * (lv + kRvLog2Pi + d * d / expf(lv));
}

__device__ inline RvKl rv_kl(float z, float mu, float lv, float pm, float plv, float om, float olv, float ulv) {
    const float a0 = rv_log_norm(z, pm, plv) + logf(3.f / 20.f), a1 = rv_log_norm(z, om, olv) + logf(3.f / 4.f),
                a2 = rv_log_norm(z, pm, ulv) + logf(1.f / 10.f);
    const float mx = fmaxf(a0, fmaxf(a1, a2));
    const float e0 = expf(a0 - mx), e1 = expf(a1 - mx), e2 = expf(a2 - mx), se = e0 + e1 + e2;
    const float d = z - mu, iv = 1.f / expf(lv);
    RvKl r;
    r.term = rv_log_norm(z, mu, lv) - (mx + logf(se));
    r.q_z = -d * iv;
    r.q_lv = -0.5f * (1.f - d * d * iv);
    r.p_z = (e0 * (-(z - pm) / expf(plv)) + e1 * (-(z - om) / expf(olv)) + e2 * (-(z - pm) / expf(ulv))) / se;
    return r;
}

// ---- latent: z and the users' weighted KL sums, one workgroup per user (k <= 256: one column per thread) -------------------------
__global__ __launch_bounds__(kVaeBlock) void rv_latent_kernel(const int32_t *__restrict__ users, int k, const float *__restrict__ mu,
                                                              const float *__restrict__ lv, const float *__restrict__ eps,
                                                              const float *__restrict__ pri, const float *__restrict__ post_mu,
                                                              const float *__restrict__ post_lv, const float *__restrict__ sumx, float gamma,
                                                              float beta, float *z, float *kld) {
    __shared__ float sh[kVaeBlock];
    const int64_t b = blockIdx.x, u = users[b];
    const int c = threadIdx.x;
    float t = 0.f;
    if (c < k) {
        const float m = mu[b * k + c], l = lv[b * k + c];
        const float zz = m + eps[u * k + c] * expf(0.5f * l);
        z[b * k + c] = zz;
        t = rv_kl(zz, m, l, pri[c], pri[k + c], post_mu[u * k + c], post_lv[u * k + c], pri[2 * k + c]).term;
    }
    t = block_sum(t, sh);
    if (threadIdx.x == 0) kld[b] = (gamma != 0.f ? gamma * sumx[u] : beta) * t;
}

// gz = the decoder's part (the item ranges' partial sums, ascending) + the KL term's; gmu, glv from z = mu + eps exp(lv / 2)
__global__ __launch_bounds__(kVaeBlock) void rv_latent_back_kernel(const int32_t *__restrict__ users, int k, int64_t nb,
                                                                   const float *__restrict__ part, int n_split, const float *__restrict__ mu,
                                                                   const float *__restrict__ lv, const float *__restrict__ z,
                                                                   const float *__restrict__ eps, const float *__restrict__ pri,
                                                                   const float *__restrict__ post_mu, const float *__restrict__ post_lv,
                                                                   const float *__restrict__ sumx, float gamma, float beta, float inv_b,
                                                                   float *gmu, float *glv) {
    const int64_t b = blockIdx.x, u = users[b];
    const int c = threadIdx.x;
    if (c >= k) return;
    float gz = 0.f;
    for (int s = 0; s < n_split; ++s) gz += part[((int64_t)s * nb + b) * k + c];
    const float m = mu[b * k + c], l = lv[b * k + c];
    const RvKl t = rv_kl(z[b * k + c], m, l, pri[c], pri[k + c], post_mu[u * k + c], post_lv[u * k + c], pri[2 * k + c]);
    const float w = (gamma != 0.f ? gamma * sumx[u] : beta) * inv_b;
    gz += w * (t.q_z - t.p_z);
    gmu[b * k + c] = gz - w * t.q_z;
    glv[b * k + c] = gz * (eps[u * k + c] * expf(0.5f * l) * 0.5f) + w * t.q_lv;
}

// ---- likelihood: one workgroup per row of the logits (recvae.py:105) ------------------------------------------------------------
// mll[b] = sum_i x_i log_softmax(o)_i; row <- dL/do = (softmax(o) sum_i x_i - x) / B
__global__ __launch_bounds__(kVaeBlock) void rv_likelihood_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx,
                                                                  const float *__restrict__ x, const float *__restrict__ sumx,
                                                                  const int32_t *__restrict__ users, float *o, int64_t I, float inv_b,
                                                                  float *mll) {
    __shared__ float sh[kVaeBlock];
    const int64_t b = blockIdx.x, u = users[b];
    const int64_t lo = row_ptr[u], hi = row_ptr[u + 1];
    float *row = o + b * I;
    float mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) mx = fmaxf(mx, row[i]);
    mx = block_max(mx, sh);
    float se = 0.f;
    for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) se += expf(row[i] - mx);
    se = block_sum(se, sh);
    const float lse = mx + logf(se);
    float ll = 0.f;
    for (int64_t e = lo + threadIdx.x; e < hi; e += kVaeBlock) ll += x[e] * (row[row_idx[e]] - lse);
    ll = block_sum(ll, sh);   // (its barriers also order the reads above before the stores below)
    if (threadIdx.x == 0) mll[b] = ll;
    const float sx = sumx[u] * inv_b;
    for (int64_t i = threadIdx.x; i < I; i += kVaeBlock) row[i] = expf(row[i] - mx) / se * sx;
    __syncthreads();
    for (int64_t e = lo + threadIdx.x; e < hi; e += kVaeBlock) row[row_idx[e]] -= x[e] * inv_b;   // (indices without repeats)
}

// ---- Adam on the vectors: g[i] = sum_b x[b n + i] (y[b n + i]), b ascending -------------------------------------------------------
struct RvVec {
    const float *x, *y;
    int64_t n, at;
};
constexpr int kRvMaxVecs = 18;
struct RvVecs {
    RvVec v[kRvMaxVecs];
};

__global__ void rv_vec_adam_kernel(float *w, float *am, float *av, RvVecs vs, int64_t nb, VaeAdam ad) {
    const RvVec d = vs.v[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    float g = 0.f;
    if (d.y) for (int64_t b = 0; b < nb; ++b) g = fmaf(d.x[b * d.n + i], d.y[b * d.n + i], g);
    else for (int64_t b = 0; b < nb; ++b) g += d.x[b * d.n + i];
    vae_adam(w, am, av, d.at + i, g, ad);
}

// ---- Adam on fc1 (one row per item): the batch's users are the positions [p0, p0 + nb) of the pass; col_pos lists every item's
// entries by ascending position, col_ent their place in the CSR ----------------------------------------------------------------
__global__ void rv_w1_adam_kernel(float *w, float *am, float *av, int64_t I, int h, int64_t p0, int64_t nb,
                                  const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ col_pos,
                                  const int64_t *__restrict__ col_ent, const float *__restrict__ xn, const uint8_t *__restrict__ keep,
                                  float scale, const float *__restrict__ gp, VaeAdam ad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= I * h) return;
    const int64_t i = e / h, j = e % h;
    int64_t lo = col_ptr[i], hi = col_ptr[i + 1];
    const int64_t end = hi;
    while (lo < hi) {   // the first of the item's entries at a position not below p0
        const int64_t mid = (lo + hi) >> 1;
        if (col_pos[mid] < p0) lo = mid + 1; else hi = mid;
    }
    float g = 0.f;
    for (; lo < end && col_pos[lo] < p0 + nb; ++lo) {
        const int64_t c = col_ent[lo];
        if (keep && !keep[c]) continue;
        const float x = keep ? xn[c] * scale : xn[c];
        g = fmaf(x, gp[((int64_t)col_pos[lo] - p0) * h + j], g);
    }
    vae_adam(w, am, av, e, g, ad);
}

__global__ void rv_iota_kernel(int32_t *out, int64_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = (int32_t)q;
}

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_recvae : ModelHandle {
    int64_t n_users = 0, n_items = 0, nnz = 0;
    int k = 0, h = 0;
    int64_t t_enc = 0, t_dec = 0;   // the two Adams' step counters
    RvLayout L{};
    // in the reference's state_dict order: the encoder's 24 tables (of w / m / v, and of `old` from 0), the three prior rows of
    // `pri`, and decoder.weight / decoder.bias of w / m / v
    std::vector<TableSlot> enc, prior, dec;
    DevCsr rows;                     // pointers and indices (values live in x / xn as float32)
    DevBuf<float> x, xn, sumx;       // the stored ratings, the L2-normalised ones, the rows' sums
    DevBuf<int64_t> col_ptr, col_ent;
    DevBuf<int32_t> col_pos, order, iota;
    std::vector<int64_t> h_ptr, h_col_ptr;   // host copies for the per-pass counting sort
    std::vector<int32_t> h_idx;
    DevBuf<float> w, m, v, old, pri, post_mu, post_lv, eps, mll, kld;
    DevBuf<uint8_t> keep;
    bool post_stale = true;
    // per call, sized for `cap` rows
    int64_t cap = 0;
    int n_split = 1, n_chunks = 1;   // item ranges of the gz product; chunks of the longest row
    int64_t kchunk = 0;
    DevBuf<float> part_in;   // the input layer's chunk sums, cap x n_chunks x h
    DevBuf<float> act;   // 5 x (pre, xhat, hid, G, gp) + R + S, each cap x h
    DevBuf<float> rstd, mu, lv, z, gmu, glv, logits, part, out;
    float *pre(int l) { return act.p + (size_t)(0 * kRvLayers + l) * (size_t)cap * (size_t)h; }
    float *xhat(int l) { return act.p + (size_t)(1 * kRvLayers + l) * (size_t)cap * (size_t)h; }
    float *hid(int l) { return act.p + (size_t)(2 * kRvLayers + l) * (size_t)cap * (size_t)h; }
    float *G(int l) { return act.p + (size_t)(3 * kRvLayers + l) * (size_t)cap * (size_t)h; }
    float *gp(int l) { return act.p + (size_t)(4 * kRvLayers + l) * (size_t)cap * (size_t)h; }
    float *R() { return act.p + (size_t)(5 * kRvLayers) * (size_t)cap * (size_t)h; }
    float *S() { return act.p + (size_t)(5 * kRvLayers + 1) * (size_t)cap * (size_t)h; }
};

// the 26 trainable tables (encoder's 24, decoder.weight, decoder.bias) of `buf` (w, m or v) to the host
static void rv_get_trainable(cornac_hip_recvae_t h, const DevBuf<float> &buf, float *const *tables) {
    get_tables(h->stream, buf.p, h->enc, tables);
    get_tables(h->stream, buf.p, h->dec, tables + kRvEncTables);
}

static void rv_ensure(cornac_hip_recvae_t h, int64_t cap) {
    if (cap <= h->cap) return;
    const size_t I = (size_t)h->n_items, hh = (size_t)h->h, k = (size_t)h->k, c = (size_t)cap;
    h->n_split = (int)std::min<int64_t>(32, std::max<int64_t>(1, (h->n_items + 1023) / 1024));
    h->kchunk = ((h->n_items + h->n_split - 1) / h->n_split + kVaeTk - 1) / kVaeTk * kVaeTk;
    const char *what = "a batch's activations and logits";
    h->cap = 0;
    alloc_named(h->act, (size_t)(5 * kRvLayers + 2) * c * hh, "RecVAE", what);
    alloc_named(h->part_in, (size_t)h->n_chunks * c * hh, "RecVAE", what);
    alloc_named(h->rstd, (size_t)kRvLayers * c, "RecVAE", what);
    for (DevBuf<float> *b : {&h->mu, &h->lv, &h->z, &h->gmu, &h->glv}) alloc_named(*b, c * k, "RecVAE", what);
    alloc_named(h->logits, c * I, "RecVAE", what);
    alloc_named(h->part, (size_t)h->n_split * c * k, "RecVAE", what);
    h->cap = cap;
}

// the encoder `enc` (the trained one or the old one) over the rows users[0 .. nb): pre / xhat / hid / rstd of every layer, mu, lv
static void rv_forward(cornac_hip_recvae_t h, const float *enc, const int32_t *users, int64_t nb, const uint8_t *keep, float scale) {
    const RvLayout &L = h->L;
    const int64_t hh = h->h, k = h->k;
    rv_input_kernel<<<dim3((unsigned)nb, (unsigned)h->n_chunks), kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, h->xn.p, keep, scale,
                                                                                           users, enc + L.W[0], (int)hh, h->part_in.p);
    rv_input_sum_kernel<<<grid(nb * hh), kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, users, h->part_in.p, h->n_chunks, enc + L.b[0], (int)hh, nb,
                                                                    h->pre(0));
    for (int l = 0; l < kRvLayers; ++l) {
        if (l > 0) linear(h->stream, "RecVAE", h->hid(l - 1), enc + L.W[l], enc + L.b[l], h->R(), nb, hh, hh, h->pre(l));
        rv_layer_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->pre(l), (int)hh, enc + L.g[l], enc + L.c[l], h->xhat(l),
                                                                  h->rstd.p + (size_t)l * (size_t)h->cap, h->hid(l), h->R(), l == 0);
    }
    linear(h->stream, "RecVAE", h->hid(kRvLayers - 1), enc + L.Wm, enc + L.bm, nullptr, nb, k, hh, h->mu.p);
    linear(h->stream, "RecVAE", h->hid(kRvLayers - 1), enc + L.Wv, enc + L.bv, nullptr, nb, k, hh, h->lv.p);
}

// the old encoder's posterior of every user (recvae.py:35), with the kernels of the training forward
static void rv_refresh_post(cornac_hip_recvae_t h) {
    if (!h->post_stale) return;
    const int64_t nu = h->n_users, k = h->k;
    rv_ensure(h, std::min<int64_t>(nu, kRvMaxBatch));
    for (int64_t u0 = 0; u0 < nu; u0 += h->cap) {
        const int64_t nb = std::min(h->cap, nu - u0);
        rv_forward(h, h->old.p, h->iota.p + u0, nb, nullptr, 1.f);
        HIP_CHECK(hipMemcpyAsync(h->post_mu.p + u0 * k, h->mu.p, (size_t)(nb * k) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        HIP_CHECK(hipMemcpyAsync(h->post_lv.p + u0 * k, h->lv.p, (size_t)(nb * k) * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->post_stale = false;
}

int cornac_hip_recvae_create(cornac_hip_recvae_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                             const int32_t *indices, const double *values, int hidden, int latent) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "RecVAE: sizes must be positive");
        REQUIRE(n_users < (1ll << 31) && n_items < (1ll << 31), "RecVAE: user and item counts must fit int32");
        REQUIRE(hidden >= 1 && hidden <= kRvMaxH, "RecVAE: hidden_dim = %d is outside the supported range 1 <= hidden_dim <= %d", hidden,
                kRvMaxH);
        REQUIRE(latent >= 1 && latent <= kRvMaxK, "RecVAE: latent_dim = %d is outside the supported range 1 <= latent_dim <= %d", latent,
                kRvMaxK);
        check_csr("RecVAE", "X", n_users, n_items, indptr, indices, values, kCsrFiniteValues);
        std::unique_ptr<cornac_hip_recvae> h(new cornac_hip_recvae());
        h->open(device);
        const int64_t nnz = indptr[n_users], I = n_items, hh = hidden, kk = latent;
        h->n_users = n_users; h->n_items = n_items; h->nnz = nnz; h->k = latent; h->h = hidden;
        {
            RvLayout &L = h->L;
            int64_t at = 0;
            // the next table, rows x cols in the reference's shape (the first layer's weight is [h x I] there, [I x h] here)
            auto add = [&](std::vector<TableSlot> &slots, int64_t rows, int64_t cols, bool transposed = false) {
                slots.push_back({at, rows, cols, transposed});
                at += rows * cols;
                return slots.back().off;
            };
            for (int l = 0; l < kRvLayers; ++l) {
                L.W[l] = add(h->enc, hh, l == 0 ? I : hh, l == 0);
                L.b[l] = add(h->enc, 1, hh);
                L.g[l] = add(h->enc, 1, hh);
                L.c[l] = add(h->enc, 1, hh);
            }
            L.Wm = add(h->enc, kk, hh);
            L.bm = add(h->enc, 1, kk);
            L.Wv = add(h->enc, kk, hh);
            L.bv = add(h->enc, 1, kk);
            L.enc_total = at;
            L.Wd = add(h->dec, I, kk);
            L.bd = add(h->dec, 1, I);
            L.total = at;
            for (int64_t q = 0; q < 3; ++q) h->prior.push_back({q * kk, 1, kk, false});
        }
        for (DevBuf<float> *b : {&h->w, &h->m, &h->v}) {
            alloc_named(*b, (size_t)h->L.total, "RecVAE", "the tables and Adam's moments");
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        alloc_named(h->old, (size_t)h->L.enc_total, "RecVAE", "the old encoder");
        HIP_CHECK(hipMemsetAsync(h->old.p, 0, h->old.n * sizeof(float), h->stream));
        alloc_named(h->pri, (size_t)(3 * kk), "RecVAE", "the prior tables");
        HIP_CHECK(hipMemsetAsync(h->pri.p, 0, h->pri.n * sizeof(float), h->stream));
        alloc_named(h->post_mu, (size_t)(n_users * kk), "RecVAE", "the old encoder's posterior");
        alloc_named(h->post_lv, (size_t)(n_users * kk), "RecVAE", "the old encoder's posterior");
        alloc_named(h->eps, (size_t)(n_users * kk), "RecVAE", "the noise");
        alloc_named(h->mll, (size_t)n_users, "RecVAE", "the users' losses");
        alloc_named(h->kld, (size_t)n_users, "RecVAE", "the users' losses");
        alloc_named(h->order, (size_t)n_users, "RecVAE", "the pass's order");
        alloc_named(h->iota, (size_t)n_users, "RecVAE", "the users' ids");
        rv_iota_kernel<<<grid(n_users), kVaeBlock, 0, h->stream>>>(h->iota.p, n_users);
        // the constants of the data set (recvae.py:67, 100): x, x / max(||x||, 1e-12) and the rows' sums, in float32
        std::vector<float> x((size_t)nnz), xn((size_t)nnz), sumx((size_t)n_users);
        int64_t longest = 0;
        for (int64_t u = 0; u < n_users; ++u) longest = std::max(longest, indptr[u + 1] - indptr[u]);
        h->n_chunks = (int)std::max<int64_t>(1, (longest + kRvChunk - 1) / kRvChunk);
        REQUIRE(h->n_chunks <= 65535, "RecVAE: a row of %lld entries is more than the input layer's grid holds", (long long)longest);
        for (int64_t u = 0; u < n_users; ++u) {
            float sq = 0.f, sm = 0.f;
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) {
                x[(size_t)e] = (float)values[e];
                sq += x[(size_t)e] * x[(size_t)e];
                sm += x[(size_t)e];
            }
            const float norm = std::max(std::sqrt(sq), 1e-12f);
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) xn[(size_t)e] = x[(size_t)e] / norm;
            sumx[(size_t)u] = sm;
        }
        h->rows.upload("RecVAE", "X", n_users, indptr, indices, nullptr, h->stream);
        alloc_named(h->x, (size_t)nnz, "RecVAE", "the ratings");
        alloc_named(h->xn, (size_t)nnz, "RecVAE", "the ratings");
        alloc_named(h->sumx, (size_t)n_users, "RecVAE", "the rows' sums");
        alloc_named(h->keep, (size_t)nnz, "RecVAE", "the dropout mask");
        alloc_named(h->col_pos, (size_t)nnz, "RecVAE", "the items' entries in the pass's order");
        alloc_named(h->col_ent, (size_t)nnz, "RecVAE", "the items' entries in the pass's order");
        alloc_named(h->col_ptr, (size_t)n_items + 1, "RecVAE", "the items' entries in the pass's order");
        if (nnz) {
            h->x.upload(x.data(), (size_t)nnz, h->stream);
            h->xn.upload(xn.data(), (size_t)nnz, h->stream);
        }
        h->sumx.upload(sumx.data(), (size_t)n_users, h->stream);
        h->h_ptr.assign(indptr, indptr + n_users + 1);
        h->h_idx.assign(indices, indices + nnz);
        h->h_col_ptr.assign((size_t)n_items + 1, 0);
        for (int64_t e = 0; e < nnz; ++e) ++h->h_col_ptr[(size_t)indices[e] + 1];
        for (int64_t i = 0; i < n_items; ++i) h->h_col_ptr[(size_t)i + 1] += h->h_col_ptr[(size_t)i];
        h->col_ptr.upload(h->h_col_ptr.data(), (size_t)n_items + 1, h->stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_recvae_destroy(cornac_hip_recvae_t h) { return destroy_handle(h); }

int cornac_hip_recvae_set_params(cornac_hip_recvae_t h, const float *const *tables) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        REQUIRE(tables != nullptr, "RecVAE: tables is NULL");
        const float *const *old = tables + kRvEncTables + 3;
        put_tables(h->stream, h->w.p, h->enc, tables);
        put_tables(h->stream, h->pri.p, h->prior, tables + kRvEncTables);   // (read per step)
        put_tables(h->stream, h->old.p, h->enc, old);
        put_tables(h->stream, h->w.p, h->dec, tables + kRvTables - 2);
        if (std::any_of(old, old + kRvEncTables, [](const float *t) { return t != nullptr; })) h->post_stale = true;
    });
}

int cornac_hip_recvae_get_params(cornac_hip_recvae_t h, float *const *tables) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        REQUIRE(tables != nullptr, "RecVAE: tables is NULL");
        get_tables(h->stream, h->w.p, h->enc, tables);
        get_tables(h->stream, h->pri.p, h->prior, tables + kRvEncTables);
        get_tables(h->stream, h->old.p, h->enc, tables + kRvEncTables + 3);
        get_tables(h->stream, h->w.p, h->dec, tables + kRvTables - 2);
    });
}

int cornac_hip_recvae_get_state(cornac_hip_recvae_t h, float *const *m, float *const *v, int64_t *t_enc, int64_t *t_dec) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        if (m) rv_get_trainable(h, h->m, m);
        if (v) rv_get_trainable(h, h->v, v);
        if (t_enc) *t_enc = h->t_enc;
        if (t_dec) *t_dec = h->t_dec;
    });
}

int cornac_hip_recvae_reset_optimizer(cornac_hip_recvae_t h) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        zero_state(h->stream, {&h->m, &h->v});
        h->t_enc = h->t_dec = 0;
    });
}

int cornac_hip_recvae_update_prior(cornac_hip_recvae_t h) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        HIP_CHECK(hipMemcpyAsync(h->old.p, h->w.p, (size_t)h->L.enc_total * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        h->post_stale = true;
        rv_refresh_post(h);
    });
}

int cornac_hip_recvae_get_prior_posterior(cornac_hip_recvae_t h, float *mu_out, float *logvar_out) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        rv_refresh_post(h);
        const size_t n = (size_t)(h->n_users * h->k);
        if (mu_out) h->post_mu.download(mu_out, n, h->stream);
        if (logvar_out) h->post_lv.download(logvar_out, n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_recvae_fit_epoch(cornac_hip_recvae_t h, const int32_t *order, int64_t batch_size, float lr, float gamma, float beta,
                                float dropout_rate, int step_encoder, int step_decoder, const uint8_t *keep, const float *eps,
                                uint64_t seed, double *step_loss) {
    return guarded([&] {
        check_handle(h, "RecVAE handle");
        REQUIRE(order != nullptr, "RecVAE: order is NULL");
        REQUIRE(batch_size >= 1 && batch_size <= kRvMaxBatch, "RecVAE: batch_size = %lld is outside the supported range 1 <= batch_size <= %d",
                (long long)batch_size, kRvMaxBatch);
        REQUIRE(std::isfinite(lr) && std::isfinite(gamma) && std::isfinite(beta), "RecVAE: lr, gamma and beta must be finite");
        REQUIRE(dropout_rate >= 0.f && dropout_rate < 1.f, "RecVAE: dropout_rate = %g is outside 0 <= dropout_rate < 1", (double)dropout_rate);
        const int64_t nu = h->n_users, I = h->n_items, hh = h->h, k = h->k, nnz = h->nnz;
        {   // order must list every user once: the positions index the batch's buffers
            std::vector<uint8_t> seen((size_t)nu, 0);
            for (int64_t p = 0; p < nu; ++p) {
                REQUIRE(order[p] >= 0 && order[p] < nu, "RecVAE: user %d out of range", order[p]);
                REQUIRE(!seen[(size_t)order[p]], "RecVAE: user %d occurs twice in the pass's order", order[p]);
                seen[(size_t)order[p]] = 1;
            }
        }
        rv_refresh_post(h);
        rv_ensure(h, std::min(batch_size, nu));
        const uint64_t key = (uint64_t)(h->t_enc + h->t_dec);
        const bool drop = dropout_rate > 0.f;
        const float scale = 1.f / (1.f - dropout_rate);
        h->order.upload(order, (size_t)nu, h->stream);
        if (drop && nnz) {
            if (keep) h->keep.upload(keep, (size_t)nnz, h->stream);
            else rv_keep_kernel<<<grid(nnz), kVaeBlock, 0, h->stream>>>(h->keep.p, nnz, 1.f - dropout_rate, key, seed);
        }
        const uint8_t *kp = drop && nnz ? h->keep.p : nullptr;
        if (eps) h->eps.upload(eps, (size_t)(nu * k), h->stream);
        else rv_noise_kernel<<<grid(nu * k), kVaeBlock, 0, h->stream>>>(h->eps.p, nu, (int)k, key, seed);
        std::vector<int32_t> col_pos;
        std::vector<int64_t> col_ent;
        if (step_encoder && nnz) {   // every item's entries by ascending position in this pass: a counting sort
            col_pos.resize((size_t)nnz);
            col_ent.resize((size_t)nnz);
            std::vector<int64_t> fill(h->h_col_ptr.begin(), h->h_col_ptr.end() - 1);
            for (int64_t p = 0; p < nu; ++p)
                for (int64_t e = h->h_ptr[(size_t)order[p]]; e < h->h_ptr[(size_t)order[p] + 1]; ++e) {
                    const int64_t d = fill[(size_t)h->h_idx[(size_t)e]]++;
                    col_pos[(size_t)d] = (int32_t)p;
                    col_ent[(size_t)d] = e;
                }
            h->col_pos.upload(col_pos.data(), (size_t)nnz, h->stream);
            h->col_ent.upload(col_ent.data(), (size_t)nnz, h->stream);
        }
        float *w = h->w.p, *am = h->m.p, *av = h->v.p;
        const RvLayout L = h->L;
        const int64_t n_steps = (nu + batch_size - 1) / batch_size;
        for (int64_t s = 0; s < n_steps; ++s) {
            const int64_t p0 = s * batch_size, nb = std::min(batch_size, nu - p0);
            const float inv_b = 1.0f / (float)nb;
            const int32_t *users = h->order.p + p0;
            rv_forward(h, w, users, nb, kp, scale);
            rv_latent_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(users, (int)k, h->mu.p, h->lv.p, h->eps.p, h->pri.p, h->post_mu.p,
                                                                       h->post_lv.p, h->sumx.p, gamma, beta, h->z.p, h->kld.p + p0);
            linear(h->stream, "RecVAE", h->z.p, w + L.Wd, w + L.bd, nullptr, nb, I, k, h->logits.p);
            rv_likelihood_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, h->x.p, h->sumx.p, users, h->logits.p, I,
                                                                           inv_b, h->mll.p + p0);
            if (step_encoder) {
                h->t_enc += 1;
                const VaeAdam ad = adam_at(h->t_enc, lr);
                // gz partials: go[nb x I] D[I x k] over n_split item ranges
                linear_back_split(h->stream, "RecVAE", h->logits.p, w + L.Wd, nb, k, I, h->kchunk, h->n_split, h->part.p);
                rv_latent_back_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(users, (int)k, nb, h->part.p, h->n_split, h->mu.p, h->lv.p,
                                                                                h->z.p, h->eps.p, h->pri.p, h->post_mu.p, h->post_lv.p,
                                                                                h->sumx.p, gamma, beta, inv_b, h->gmu.p, h->glv.p);
                const int top = kRvLayers - 1;
                linear_back(h->stream, "RecVAE", h->gmu.p, w + L.Wm, nullptr, nb, hh, k, h->G(top));
                linear_back(h->stream, "RecVAE", h->glv.p, w + L.Wv, h->G(top), nb, hh, k, h->G(top));
                for (int l = top; l >= 0; --l) {
                    rv_layer_back_kernel<<<(unsigned)nb, kVaeBlock, 0, h->stream>>>(h->G(l), h->pre(l), h->xhat(l),
                                                                                   h->rstd.p + (size_t)l * (size_t)h->cap, (int)hh, w + L.g[l],
                                                                                   h->gp(l), h->S(), l == top);
                    if (l > 0) linear_back(h->stream, "RecVAE", h->gp(l), w + L.W[l], h->S(), nb, hh, hh, h->G(l - 1));
                }
                // every gradient is taken: now the encoder's Adam
                RvVecs vs{};
                int nv = 0;
                for (int l = 0; l < kRvLayers; ++l) {
                    vs.v[nv++] = RvVec{h->gp(l), nullptr, hh, L.b[l]};
                    vs.v[nv++] = RvVec{h->G(l), h->xhat(l), hh, L.g[l]};
                    vs.v[nv++] = RvVec{h->G(l), nullptr, hh, L.c[l]};
                }
                vs.v[nv++] = RvVec{h->gmu.p, nullptr, k, L.bm};
                vs.v[nv++] = RvVec{h->glv.p, nullptr, k, L.bv};
                rv_vec_adam_kernel<<<dim3(grid(std::max(hh, k)), (unsigned)nv), kVaeBlock, 0, h->stream>>>(w, am, av, vs, nb, ad);
                for (int l = 1; l < kRvLayers; ++l)
                    weight_adam(h->stream, "RecVAE", h->gp(l), h->hid(l - 1), nb, hh, hh, w + L.W[l], am + L.W[l], av + L.W[l], ad);
                weight_adam(h->stream, "RecVAE", h->gmu.p, h->hid(top), nb, k, hh, w + L.Wm, am + L.Wm, av + L.Wm, ad);
                weight_adam(h->stream, "RecVAE", h->glv.p, h->hid(top), nb, k, hh, w + L.Wv, am + L.Wv, av + L.Wv, ad);
                rv_w1_adam_kernel<<<grid(I * hh), kVaeBlock, 0, h->stream>>>(w + L.W[0], am + L.W[0], av + L.W[0], I, (int)hh, p0, nb,
                                                                             h->col_ptr.p, h->col_pos.p, h->col_ent.p, h->xn.p, kp, scale,
                                                                             h->gp(0), ad);
            }
            if (step_decoder) {
                h->t_dec += 1;
                const VaeAdam ad = adam_at(h->t_dec, lr);
                RvVecs vs{};
                vs.v[0] = RvVec{h->logits.p, nullptr, I, L.bd};
                rv_vec_adam_kernel<<<dim3(grid(I), 1), kVaeBlock, 0, h->stream>>>(w, am, av, vs, nb, ad);
                weight_adam(h->stream, "RecVAE", h->logits.p, h->z.p, nb, I, k, w + L.Wd, am + L.Wd, av + L.Wd, ad);
            }
            HIP_CHECK(hipGetLastError());
        }
        std::vector<float> mll((size_t)nu), kld((size_t)nu);
        h->mll.download(mll.data(), (size_t)nu, h->stream);
        h->kld.download(kld.data(), (size_t)nu, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int64_t s = 0; step_loss && s < n_steps; ++s) {
            const int64_t p0 = s * batch_size, nb = std::min(batch_size, nu - p0);
            double a = 0.0, c = 0.0;
            for (int64_t b = 0; b < nb; ++b) {
                a += (double)mll[(size_t)(p0 + b)];
                c += (double)kld[(size_t)(p0 + b)];
            }
            a /= (double)nb;
            c /= (double)nb;
            step_loss[3 * s] = a;
            step_loss[3 * s + 1] = c;
            step_loss[3 * s + 2] = -(a - c);
        }
    });
}

// users[0 .. n) in chunks: the encoder without dropout; then mu (and logvar) to the host (what == 0), the logits' rows at
// z = mu (1) or their entries items[q] (2)
static void rv_predict(cornac_hip_recvae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out, float *out2, int what) {
    check_handle(h, "RecVAE handle");
    check_ids("RecVAE", users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t I = h->n_items, k = h->k;
    const int64_t B = std::min<int64_t>(n, std::max<int64_t>(1, std::min<int64_t>(kRvMaxBatch, kRvScoreBytes / (4 * I))));
    rv_ensure(h, B);
    if (items && h->out.n < (size_t)B) alloc_named(h->out, (size_t)B, "RecVAE", "the scores");
    for_each_chunk("RecVAE", *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        rv_forward(h, h->w.p, h->user_ids.p, nb, nullptr, 1.f);
        if (what == 0) {
            h->mu.download(out + b0 * k, (size_t)(nb * k), h->stream);
            if (out2) h->lv.download(out2 + b0 * k, (size_t)(nb * k), h->stream);
            return;
        }
        linear(h->stream, "RecVAE", h->mu.p, h->w.p + h->L.Wd, h->w.p + h->L.bd, nullptr, nb, I, k, h->logits.p);
        if (what == 1) {
            h->logits.download(out + b0 * I, (size_t)(nb * I), h->stream);
        } else {
            gather_pairs_kernel<<<grid(nb), kVaeBlock, 0, h->stream>>>(h->logits.p, I, h->item_ids.p, nb, h->out.p);
            h->out.download(out + b0, (size_t)nb, h->stream);
        }
    });
}

int cornac_hip_recvae_encode_users(cornac_hip_recvae_t h, const int32_t *users, int64_t n, float *mu_out, float *logvar_out) {
    return guarded([&] { rv_predict(h, users, nullptr, n, mu_out, logvar_out, 0); });
}

int cornac_hip_recvae_score_users(cornac_hip_recvae_t h, const int32_t *users, int64_t n, float *out) {
    return guarded([&] { rv_predict(h, users, nullptr, n, out, nullptr, 1); });
}

int cornac_hip_recvae_score_pairs(cornac_hip_recvae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "RecVAE: items is NULL");
        rv_predict(h, users, items, n, out, nullptr, 2);
    });
}

// Neural collaborative filtering (He et al. 2017; cornac/models/ncf/backend_pt.py:22-175, recom_ncf_base.py:240-293) on
// gfx950, float32 throughout: GMF, MLP and NeuMF behind one handle.  The handle owns the training CSR with its values (for
// the sampler), the model's tables under the reference's state_dict order in one buffer, two state buffers of the same
// layout for the learner (adam: exp_avg, exp_avg_sq; rmsprop: square_avg; adagrad: sum; sgd: none), and one step counter.
//
// An epoch's samples (users, items, labels, cut into steps by step_ptr) lie on the device before the first step: uploaded
// once (fit_epoch) or drawn there (fit_epoch_sampled).  Then, with no host synchronisation in between:
//   order      once per epoch, all steps in one launch: each step's samples sorted by user id and by item id, stable, by
//              counting (a sample's place = the ids below it + the equal ids before it); at most 16 384 ids per step
//   per step   forward/backward  one workgroup per 8 samples: gather the embedding rows, h_gmf = p q, the layers (each
//                         output one ascending fmaf chain), the logit over [h_gmf | h_mlp], p, the BCE term, dL/dlogit as
//                         torch computes it, the chain back through the layers; activations, their derivatives and the
//                         per-sample gradients go to global memory
//              sweep      one thread per entry of every table that has a gradient: an embedding entry finds its row in
//                         the step's sorted ids by bisection and sums its samples' gradients in sample order; a weight,
//                         bias or logit entry sums over the step's samples in 16 interleaved slices, one thread each,
//                         combined in ascending slice order (these sums are float64, rounded once: a float32 chain
//                         over 1 280 samples costs exp_avg_sq its last bits); then g += reg p and the learner's dense
//                         update.  NeuMF's gmf.logit / mlp.logit have no gradient and are not visited.
//   losses     once per epoch: each step's terms summed by a fixed tree in float64
// No float atomics and no atomics at all; every sum has one fixed order, so the same inputs give the same bits.
//
// The sampler (draw): position k of the epoch takes the stored entry feistel_perm(k) (keyed by seed and epoch); each
// positive is followed, in the reference's layout [positives | negatives, user-major], by num_neg items uniform among those
// j for which (u, j) is not stored with a value > 0: kNcfTries Philox draws (keyed by seed, epoch, sample, try), then, if
// all were refused, exactly the r-th admissible item, r uniform, by a walk over the row's entries.  No unbounded loop.
#include "rng.h"
#include "vae_host.h"

namespace chip {
namespace {

constexpr int kNcfMaxF = 256, kNcfMaxL0 = 512, kNcfMaxW = 256, kNcfMaxLayers = 8, kNcfMaxStep = 16384;
constexpr int kNcfTile = 8;          // samples per workgroup of the forward / backward kernel
constexpr int kNcfTries = 16;        // rejected draws before the exact walk
constexpr int kNcfSlices = 16;       // interleaved slices of a weight entry's sum over the step's samples
constexpr int kNcfMaxTables = 6 + 2 * (kNcfMaxLayers - 1) + 4;
constexpr int64_t kNcfScoreBytes = 256ll << 20;   // a scoring chunk's probabilities
constexpr int64_t kNcfScoreUsers = 1024, kNcfScorePairs = 4096;
enum { NCF_GMF = 0, NCF_MLP, NCF_NEUMF, NCF_KINDS };
enum { NCF_ADAM = 0, NCF_SGD, NCF_RMSPROP, NCF_ADAGRAD, NCF_LEARNERS };
enum { NACT_SIGMOID = 0, NACT_TANH, NACT_ELU, NACT_SELU, NACT_RELU, NACT_RELU6, NACT_LEAKY, NACT_COUNT };
// what a table is to the sweep
enum { ROLE_NONE = 0, ROLE_GMF_U, ROLE_GMF_I, ROLE_MLP_U, ROLE_MLP_I, ROLE_W, ROLE_B, ROLE_LOGIT_W, ROLE_LOGIT_B };

// the network as the kernels see it; offsets (floats) into the parameter buffer
struct NcfNet {
    int kind, F, nl, act;                 // F: GMF's factors (0 for MLP); nl: len(layers) (0 for GMF)
    int width[kNcfMaxLayers];
    int act_off[kNcfMaxLayers];           // where layer l's values start in a sample's record of `sumw` floats
    int sumw;
    int64_t w_off[kNcfMaxLayers], b_off[kNcfMaxLayers];   // layer l: W [width[l + 1] x width[l]], b [width[l + 1]]
    int64_t gmf_u, gmf_i, mlp_u, mlp_i;   // the embedding tables
    int64_t logit_w, logit_b;             // the logit that forward() uses
};

struct NcfTable {
    int64_t off, rows, cols;
    int role, layer;
};

struct NcfTables {
    int n;
    NcfTable t[kNcfMaxTables];
};

struct NcfOpt {
    int learner;
    float lr, reg;
    VaeAdam adam;
};

// selu and leaky_relu (slope 0.01) beside vae_act's five, which keep their numbering and arithmetic
__device__ inline float ncf_act(int act, float x, float *d) {
    switch (act) {
    case NACT_SIGMOID: return vae_act(ACT_SIGMOID, x, d);
    case NACT_TANH: return vae_act(ACT_TANH, x, d);
    case NACT_ELU: return vae_act(ACT_ELU, x, d);
    case NACT_RELU: return vae_act(ACT_RELU, x, d);
    case NACT_RELU6: return vae_act(ACT_RELU6, x, d);
    case NACT_SELU: {
        const float scale = 1.0507009873554804934193349852946f, alpha = 1.6732632423543772848170429916717f;
        if (x > 0.f) { *d = scale; return scale * x; }
        *d = scale * alpha * expf(x);
        return scale * alpha * expm1f(x);
    }
    default: *d = x > 0.f ? 1.f : 0.01f; return x > 0.f ? x : 0.01f * x;
    }
}

// ---- order: a step's samples sorted by id, stable --------------------------------------------------------------------------
// grid (steps, ceil(max step / 256), 2): z = 0 sorts by user, 1 by item.  order[base + place] = the sample's index in its
// step, sorted[base + place] = its id.
__global__ __launch_bounds__(kVaeBlock) void ncf_order_kernel(const int64_t *__restrict__ step_ptr, const int32_t *__restrict__ users,
                                                              const int32_t *__restrict__ items, int32_t *order_u, int32_t *sorted_u,
                                                              int32_t *order_i, int32_t *sorted_i) {
    __shared__ int32_t sh[kVaeBlock];
    const int64_t base = step_ptr[blockIdx.x];
    const int n = (int)(step_ptr[blockIdx.x + 1] - base);
    if ((int)blockIdx.y * kVaeBlock >= n) return;
    const int32_t *ids = (blockIdx.z ? items : users) + base;
    const int s = (int)blockIdx.y * kVaeBlock + (int)threadIdx.x;
    const int32_t mine = s < n ? ids[s] : 0;
    int place = 0;
    for (int t0 = 0; t0 < n; t0 += kVaeBlock) {
        sh[threadIdx.x] = t0 + (int)threadIdx.x < n ? ids[t0 + threadIdx.x] : 0;
        __syncthreads();
        const int m = n - t0 < kVaeBlock ? n - t0 : kVaeBlock;
        for (int t = 0; t < m; ++t) {
            const int32_t o = sh[t];
            place += (o < mine || (o == mine && t0 + t < s)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (s < n) {
        (blockIdx.z ? order_i : order_u)[base + place] = s;
        (blockIdx.z ? sorted_i : sorted_u)[base + place] = mine;
    }
}

// ---- forward (and backward): one workgroup per kNcfTile samples ----------------------------------------------------------------
// Sample q of [0, n): (users[q], items[q]), or, with items == NULL, (users[q / n_items], q % n_items): a scoring chunk's
// rows.  TRAIN: writes the sample's record of activations (hbuf), derivatives (dbuf) and pre-activation gradients (gabuf;
// its layer-0 part is the gradient of the concatenated embedding input), h_gmf and the GMF rows' gradients, dL/dlogit and
// the loss term.  Otherwise writes p to out[q].
template <bool TRAIN>
__global__ __launch_bounds__(kVaeBlock) void ncf_forward_kernel(NcfNet N, const float *__restrict__ w, const int32_t *__restrict__ users,
                                                                const int32_t *__restrict__ items, int64_t n_items, int64_t n,
                                                                const float *__restrict__ labels, float inv_n, float *out, float *hbuf,
                                                                float *dbuf, float *gabuf, float *hg, float *gu, float *gi, float *dl,
                                                                float *loss) {
    __shared__ float sA[kNcfTile][kNcfMaxL0];
    __shared__ float sB[kNcfTile][kNcfMaxW];
    __shared__ float sG[kNcfTile][kNcfMaxF];
    __shared__ int32_t s_u[kNcfTile], s_i[kNcfTile];
    __shared__ float s_dl[kNcfTile];
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kNcfTile;
    const int nt = (int)(n - q0 < kNcfTile ? n - q0 : kNcfTile);
    if (tid < nt) {
        const int64_t q = q0 + tid;
        s_u[tid] = items ? users[q] : users[q / n_items];
        s_i[tid] = items ? items[q] : (int32_t)(q % n_items);
    }
    __syncthreads();
    const int F = N.F, nl = N.nl;
    for (int idx = tid; idx < nt * F; idx += kVaeBlock) {
        const int s = idx / F, f = idx % F;
        const float v = w[N.gmf_u + (int64_t)s_u[s] * F + f] * w[N.gmf_i + (int64_t)s_i[s] * F + f];
        sG[s][f] = v;
        if (TRAIN) hg[(q0 + s) * F + f] = v;
    }
    if (nl) {
        const int L0 = N.width[0], half = L0 / 2;
        for (int idx = tid; idx < nt * L0; idx += kVaeBlock) {
            const int s = idx / L0, c = idx % L0;
            const float v = c < half ? w[N.mlp_u + (int64_t)s_u[s] * half + c] : w[N.mlp_i + (int64_t)s_i[s] * half + (c - half)];
            sA[s][c] = v;
            if (TRAIN) hbuf[(q0 + s) * N.sumw + c] = v;
        }
    }
    __syncthreads();
    for (int l = 0; l + 1 < nl; ++l) {
        const int in = N.width[l], on = N.width[l + 1];
        const float *x = (l & 1) ? &sB[0][0] : &sA[0][0];
        float *y = (l & 1) ? &sA[0][0] : &sB[0][0];
        const int xs = (l & 1) ? kNcfMaxW : kNcfMaxL0, ys = (l & 1) ? kNcfMaxL0 : kNcfMaxW;
        const float *W = w + N.w_off[l], *b = w + N.b_off[l];
        for (int idx = tid; idx < nt * on; idx += kVaeBlock) {
            const int s = idx / on, j = idx % on;
            const float *wr = W + (int64_t)j * in, *xr = x + s * xs;
            float a = 0.f;
            for (int k = 0; k < in; ++k) a = fmaf(xr[k], wr[k], a);
            a += b[j];
            float d;
            const float v = ncf_act(N.act, a, &d);
            y[s * ys + j] = v;
            if (TRAIN) {
                hbuf[(q0 + s) * N.sumw + N.act_off[l + 1] + j] = v;
                dbuf[(q0 + s) * N.sumw + N.act_off[l + 1] + j] = d;
            }
        }
        __syncthreads();
    }
    // the last layer's values: layer nl - 1 lies where layer nl - 2 wrote it
    const float *hl = ((nl - 2) & 1) ? &sA[0][0] : &sB[0][0];
    const int hs = ((nl - 2) & 1) ? kNcfMaxL0 : kNcfMaxW;
    const int last = nl ? N.width[nl - 1] : 0;
    const float *lw = w + N.logit_w;
    if (tid < nt) {
        const int s = tid;
        float a = 0.f;
        for (int f = 0; f < F; ++f) a = fmaf(sG[s][f], lw[f], a);
        for (int j = 0; j < last; ++j) a = fmaf(hl[s * hs + j], lw[F + j], a);
        a += w[N.logit_b];
        const float p = 1.f / (1.f + expf(-a));
        if (!TRAIN) {
            out[q0 + s] = p;
        } else {
            const float y = labels[q0 + s];
            loss[q0 + s] = -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(logf(1.f - p), -100.f));
            const float pq = (1.f - p) * p;
            const float g = inv_n * (p - y) / fmaxf(pq, 1e-12f) * pq;   // BCELoss's backward, then the sigmoid's
            s_dl[s] = g;
            dl[q0 + s] = g;
        }
    }
    if (!TRAIN) return;
    __syncthreads();
    for (int idx = tid; idx < nt * F; idx += kVaeBlock) {
        const int s = idx / F, f = idx % F;
        const float gh = s_dl[s] * lw[f];
        gu[(q0 + s) * F + f] = gh * w[N.gmf_i + (int64_t)s_i[s] * F + f];
        gi[(q0 + s) * F + f] = gh * w[N.gmf_u + (int64_t)s_u[s] * F + f];
    }
    if (!nl) return;
    // gh of the last layer, where its values were
    {
        float *g = ((nl - 2) & 1) ? &sA[0][0] : &sB[0][0];
        for (int idx = tid; idx < nt * last; idx += kVaeBlock) {
            const int s = idx / last, j = idx % last;
            g[s * hs + j] = s_dl[s] * lw[F + j];
        }
    }
    __syncthreads();
    for (int l = nl - 2; l >= 0; --l) {
        const int in = N.width[l], on = N.width[l + 1];
        float *g = (l & 1) ? &sA[0][0] : &sB[0][0];     // gradient of layer l + 1's values, then of its pre-activations
        float *gp = (l & 1) ? &sB[0][0] : &sA[0][0];    // gradient of layer l's values
        const int gs = (l & 1) ? kNcfMaxL0 : kNcfMaxW, ps = (l & 1) ? kNcfMaxW : kNcfMaxL0;
        for (int idx = tid; idx < nt * on; idx += kVaeBlock) {
            const int s = idx / on, j = idx % on;
            const int64_t at = (q0 + s) * N.sumw + N.act_off[l + 1] + j;
            const float ga = g[s * gs + j] * dbuf[at];
            g[s * gs + j] = ga;
            gabuf[at] = ga;
        }
        __syncthreads();
        const float *W = w + N.w_off[l];
        for (int idx = tid; idx < nt * in; idx += kVaeBlock) {
            const int s = idx / in, k = idx % in;
            float a = 0.f;
            for (int j = 0; j < on; ++j) a = fmaf(g[s * gs + j], W[(int64_t)j * in + k], a);
            gp[s * ps + k] = a;
            if (l == 0) gabuf[(q0 + s) * N.sumw + k] = a;
        }
        __syncthreads();
    }
}

// ---- sweep: the gradient of one entry over the step, weight decay, the learner ----------------------------------------------------
__device__ inline float ncf_row_sum(const int32_t *__restrict__ sorted, const int32_t *__restrict__ order, int n, int32_t row,
                                    const float *__restrict__ src, int64_t stride) {
    int lo = 0, hi = n;
    while (lo < hi) {   // the first place whose id is not below `row`
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < row) lo = mid + 1; else hi = mid;
    }
    double g = 0.0;
    for (; lo < n && sorted[lo] == row; ++lo) g += (double)src[(int64_t)order[lo] * stride];
    return (float)g;
}

// the learner's update of one entry with gradient g (weight decay first)
__device__ inline void ncf_apply(float *w, float *s1, float *s2, int64_t at, float g, const NcfOpt &opt) {
    const float p = w[at];
    if (opt.reg != 0.f) g = g + opt.reg * p;
    switch (opt.learner) {
    case NCF_ADAM: vae_adam(w, s1, s2, at, g, opt.adam); break;
    case NCF_SGD: w[at] = p - opt.lr * g; break;
    case NCF_RMSPROP: {
        const float sq = s1[at] * 0.99f + (float)(1.0 - 0.99) * g * g;
        s1[at] = sq;
        w[at] = p - opt.lr * (g / (sqrtf(sq) + 1e-8f));
        break;
    }
    default: {
        const float sum = s1[at] + g * g;
        s1[at] = sum;
        w[at] = p - opt.lr * (g / (sqrtf(sum) + 1e-10f));
    }
    }
}

// sum over the samples s = slice, slice + kNcfSlices, .. of a[s as] * x[s xs] (x == NULL: of a[s as]), float64
__device__ inline double ncf_slice_dot(const float *__restrict__ a, int64_t as, const float *__restrict__ x, int64_t xs, int slice, int n) {
    double acc = 0.0;
    if (x) {
#pragma unroll 4
        for (int s = slice; s < n; s += kNcfSlices) acc += (double)a[(int64_t)s * as] * (double)x[(int64_t)s * xs];
    } else {
#pragma unroll 4
        for (int s = slice; s < n; s += kNcfSlices) acc += (double)a[(int64_t)s * as];
    }
    return acc;
}

// The first ceil(small_total / 16) workgroups take the weight, bias and logit tables (S), 16 entries each: an entry's sum
// over the step's samples is cut into kNcfSlices interleaved slices, one thread each, combined in ascending slice order.  The
// other workgroups take the embedding tables (E), one thread per entry.
__global__ __launch_bounds__(kVaeBlock) void ncf_sweep_kernel(NcfNet N, NcfTables E, int64_t emb_total, NcfTables S, int64_t small_total,
                                                              float *w, float *s1, float *s2, int n, const int32_t *__restrict__ order_u,
                                                              const int32_t *__restrict__ sorted_u, const int32_t *__restrict__ order_i,
                                                              const int32_t *__restrict__ sorted_i, const float *__restrict__ hbuf,
                                                              const float *__restrict__ gabuf, const float *__restrict__ hg,
                                                              const float *__restrict__ gu, const float *__restrict__ gi,
                                                              const float *__restrict__ dl, NcfOpt opt) {
    __shared__ double part[kNcfSlices][kNcfSlices + 1];
    const int sw = N.sumw;
    const int64_t small_blocks = (small_total + kNcfSlices - 1) / kNcfSlices;
    if ((int64_t)blockIdx.x < small_blocks) {
        const int le = (int)threadIdx.x % kNcfSlices, slice = (int)threadIdx.x / kNcfSlices;
        int64_t e = (int64_t)blockIdx.x * kNcfSlices + le;
        const bool live = e < small_total;
        double acc = 0.0;
        int64_t at = 0;
        if (live) {
            int q = 0;
            while (e >= S.t[q].rows * S.t[q].cols) { e -= S.t[q].rows * S.t[q].cols; ++q; }
            const NcfTable tb = S.t[q];
            const int64_t r = e / tb.cols, c = e % tb.cols;
            at = tb.off + e;
            switch (tb.role) {
            case ROLE_W: acc = ncf_slice_dot(gabuf + N.act_off[tb.layer + 1] + r, sw, hbuf + N.act_off[tb.layer] + c, sw, slice, n); break;
            case ROLE_B: acc = ncf_slice_dot(gabuf + N.act_off[tb.layer + 1] + c, sw, nullptr, 0, slice, n); break;
            case ROLE_LOGIT_W:
                acc = c < N.F ? ncf_slice_dot(dl, 1, hg + c, N.F, slice, n)
                              : ncf_slice_dot(dl, 1, hbuf + N.act_off[N.nl - 1] + (c - N.F), sw, slice, n);
                break;
            default: acc = ncf_slice_dot(dl, 1, nullptr, 0, slice, n);
            }
        }
        part[slice][le] = acc;
        __syncthreads();
        if (slice == 0 && live) {
            double sum = 0.0;
            for (int q = 0; q < kNcfSlices; ++q) sum += part[q][le];
            ncf_apply(w, s1, s2, at, (float)sum, opt);
        }
        return;
    }
    int64_t e = ((int64_t)blockIdx.x - small_blocks) * blockDim.x + threadIdx.x;
    if (e >= emb_total) return;
    int q = 0;
    while (e >= E.t[q].rows * E.t[q].cols) { e -= E.t[q].rows * E.t[q].cols; ++q; }   // (emb_total is the sum: q stays below E.n)
    const NcfTable tb = E.t[q];
    const int64_t r = e / tb.cols, c = e % tb.cols;
    const int half = N.nl ? N.width[0] / 2 : 0;
    float g;
    switch (tb.role) {
    case ROLE_GMF_U: g = ncf_row_sum(sorted_u, order_u, n, (int32_t)r, gu + c, N.F); break;
    case ROLE_GMF_I: g = ncf_row_sum(sorted_i, order_i, n, (int32_t)r, gi + c, N.F); break;
    case ROLE_MLP_U: g = ncf_row_sum(sorted_u, order_u, n, (int32_t)r, gabuf + c, sw); break;
    default: g = ncf_row_sum(sorted_i, order_i, n, (int32_t)r, gabuf + half + c, sw);
    }
    ncf_apply(w, s1, s2, tb.off + e, g, opt);
}

// ---- losses: one workgroup per step, a fixed tree in float64 ------------------------------------------------------------------------
__global__ __launch_bounds__(kVaeBlock) void ncf_loss_kernel(const int64_t *__restrict__ step_ptr, const float *__restrict__ loss, double *step_loss) {
    __shared__ double sh[kVaeBlock];
    const int64_t lo = step_ptr[blockIdx.x], hi = step_ptr[blockIdx.x + 1];
    double a = 0.0;
    for (int64_t s = lo + threadIdx.x; s < hi; s += kVaeBlock) a += (double)loss[s];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = kVaeBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) step_loss[blockIdx.x] = sh[0] / (double)(hi - lo);
}

// ---- the sampler -----------------------------------------------------------------------------------------------------------------
// is (u, j) stored with a value > 0
__device__ inline bool ncf_positive(const int32_t *__restrict__ idx, const double *__restrict__ val, int64_t lo, int64_t hi, int32_t j) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo < end && idx[lo] == j && val[lo] > 0.0;
}

// one thread per sample of the epoch: position k < nnz of the epoch's order and slot t (0: the positive, 1 .. num_neg: a negative)
__global__ __launch_bounds__(kVaeBlock) void ncf_draw_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx,
                                                             const double *__restrict__ row_val, const int32_t *__restrict__ ent_user,
                                                             const int32_t *__restrict__ n_pos, int64_t nnz, int64_t n_items,
                                                             int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch,
                                                             int32_t *users, int32_t *items, float *labels) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = 1 + num_neg;
    if (e >= nnz * per) return;
    const int64_t k = e / per;
    const int t = (int)(e % per);
    const uint32_t key = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x9E3779B9u) ^ mix32((uint32_t)epoch * 0x85EBCA6Bu + 0x165667B1u));
    const int64_t ent = (int64_t)feistel_perm((uint32_t)k, (uint32_t)nnz, key);
    const int32_t u = ent_user[ent];
    const int64_t step = k / batch_size, b = k % batch_size;
    const int64_t nb = nnz - step * batch_size < batch_size ? nnz - step * batch_size : batch_size;
    const int64_t base = step * batch_size * per;
    if (t == 0) {
        users[base + b] = u;
        items[base + b] = row_idx[ent];
        labels[base + b] = 1.f;
        return;
    }
    const int64_t at = base + nb + b * num_neg + (t - 1);
    const int64_t lo = row_ptr[u], hi = row_ptr[u + 1];
    const uint64_t sample = (uint64_t)k * (uint64_t)num_neg + (uint64_t)(t - 1);
    const uint32_t I = (uint32_t)n_items, thresh = lemire_thresh(I);
    uint32_t r[4];
    int32_t j = -1;
    for (int tr = 0; tr < kNcfTries; ++tr) {
        philox4x32_10((uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)tr, (uint32_t)epoch, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const int32_t c = (int32_t)lemire_bounded2(r[0], r[1], I, thresh);
        if (!ncf_positive(row_idx, row_val, lo, hi, c)) { j = c; break; }
    }
    if (j < 0) {   // the r-th admissible item, r uniform: step over the row's positive entries below it
        const uint32_t A = I - (uint32_t)n_pos[u];   // > 0: checked on the host
        philox4x32_10((uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)kNcfTries, (uint32_t)epoch, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        int64_t c = (int64_t)lemire_bounded2(r[0], r[1], A, lemire_thresh(A));
        for (int64_t x = lo; x < hi; ++x) {
            if (!(row_val[x] > 0.0)) continue;
            if ((int64_t)row_idx[x] <= c) ++c; else break;
        }
        j = (int32_t)c;
    }
    users[at] = u;
    items[at] = j;
    labels[at] = 0.f;
}

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_ncf : ModelHandle {
    int64_t n_users = 0, n_items = 0, nnz = 0;
    NcfNet N{};
    NcfTables all{}, emb{}, small{};   // every table in state_dict order; those with a gradient: the embeddings, the others
    std::vector<TableSlot> slots;      // `all` as the host copies take it
    int64_t total = 0, emb_total = 0, small_total = 0;
    int64_t t = 0;             // the optimiser's step counter
    int64_t no_negative_user = -1;   // the first user with stored entries and no admissible negative
    DevCsr rows;
    DevBuf<int32_t> ent_user, n_pos;
    DevBuf<float> w, s1, s2;
    // an epoch's samples
    int64_t cap_samples = 0, cap_steps = 0;
    DevBuf<int32_t> users, items, order_u, sorted_u, order_i, sorted_i;
    DevBuf<float> labels, loss;
    DevBuf<int64_t> step_ptr;
    DevBuf<double> step_loss;
    // a step's records
    int64_t cap_step = 0;
    DevBuf<float> hbuf, dbuf, gabuf, hg, gu, gi, dl;
    DevBuf<float> out;
};

static const char *const kNcfKindName[NCF_KINDS] = {"GMF", "MLP", "NeuMF"};

static int ncf_n_tables(int kind, int n_layers) {
    const int gmf = 4, mlp = 4 + 2 * (n_layers - 1);
    return kind == NCF_GMF ? gmf : kind == NCF_MLP ? mlp : 2 + gmf + mlp;
}

// the tables in the reference's state_dict order (backend_pt.py:33-36, 73-84, 141-147), with their roles in `kind`
static void ncf_layout(cornac_hip_ncf_t h) {
    NcfNet &N = h->N;
    NcfTables &T = h->all;
    T.n = 0;
    int64_t off = 0;
    auto add = [&](int64_t rows, int64_t cols, int role, int layer) {
        NcfTable &t = T.t[T.n++];
        t.off = off; t.rows = rows; t.cols = cols; t.role = role; t.layer = layer;
        off += rows * cols;
        return t.off;
    };
    const bool neumf = N.kind == NCF_NEUMF;
    const int last = N.nl ? N.width[N.nl - 1] : 0;
    if (neumf) {
        N.logit_w = add(1, N.F + last, ROLE_LOGIT_W, 0);
        N.logit_b = add(1, 1, ROLE_LOGIT_B, 0);
    }
    if (N.kind != NCF_MLP) {
        N.gmf_u = add(h->n_users, N.F, ROLE_GMF_U, 0);
        N.gmf_i = add(h->n_items, N.F, ROLE_GMF_I, 0);
        const int64_t lw = add(1, N.F, neumf ? ROLE_NONE : ROLE_LOGIT_W, 0), lb = add(1, 1, neumf ? ROLE_NONE : ROLE_LOGIT_B, 0);
        if (!neumf) { N.logit_w = lw; N.logit_b = lb; }
    }
    if (N.kind != NCF_GMF) {
        N.mlp_u = add(h->n_users, N.width[0] / 2, ROLE_MLP_U, 0);
        N.mlp_i = add(h->n_items, N.width[0] / 2, ROLE_MLP_I, 0);
        for (int l = 0; l + 1 < N.nl; ++l) {
            N.w_off[l] = add(N.width[l + 1], N.width[l], ROLE_W, l);
            N.b_off[l] = add(1, N.width[l + 1], ROLE_B, l);
        }
        const int64_t lw = add(1, last, neumf ? ROLE_NONE : ROLE_LOGIT_W, 0), lb = add(1, 1, neumf ? ROLE_NONE : ROLE_LOGIT_B, 0);
        if (!neumf) { N.logit_w = lw; N.logit_b = lb; }
    }
    h->total = off;
    for (int q = 0; q < T.n; ++q) h->slots.push_back({T.t[q].off, T.t[q].rows, T.t[q].cols, false});
    h->emb.n = h->small.n = 0;
    h->emb_total = h->small_total = 0;
    for (int q = 0; q < T.n; ++q) {
        const int role = T.t[q].role;
        if (role == ROLE_NONE) continue;
        const bool e = role == ROLE_GMF_U || role == ROLE_GMF_I || role == ROLE_MLP_U || role == ROLE_MLP_I;
        NcfTables &L = e ? h->emb : h->small;
        L.t[L.n++] = T.t[q];
        (e ? h->emb_total : h->small_total) += T.t[q].rows * T.t[q].cols;
    }
    N.sumw = 0;
    for (int l = 0; l < N.nl; ++l) { N.act_off[l] = N.sumw; N.sumw += N.width[l]; }
}

int cornac_hip_ncf_create(cornac_hip_ncf_t *out, int device, int kind, int64_t n_users, int64_t n_items, const int64_t *indptr,
                          const int32_t *indices, const double *data, int num_factors, const int *layers, int n_layers, int act) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(kind >= 0 && kind < NCF_KINDS, "NCF: unknown model kind %d", kind);
        const char *nm = kNcfKindName[kind];
        REQUIRE(n_users > 0 && n_items > 0, "%s: sizes must be positive", nm);
        REQUIRE(n_users < (1ll << 31) && n_items < (1ll << 31), "%s: user and item counts must fit int32", nm);
        if (kind != NCF_MLP)
            REQUIRE(num_factors >= 1 && num_factors <= kNcfMaxF, "%s: num_factors = %d is outside the supported range 1 <= num_factors <= %d",
                    nm, num_factors, kNcfMaxF);
        if (kind != NCF_GMF) {
            REQUIRE(layers != nullptr && n_layers >= 2 && n_layers <= kNcfMaxLayers,
                    "%s: len(layers) = %d is outside the supported range 2 <= len(layers) <= %d", nm, layers ? n_layers : 0, kNcfMaxLayers);
            REQUIRE(layers[0] >= 2 && layers[0] <= kNcfMaxL0 && layers[0] % 2 == 0,
                    "%s: layers[0] = %d must be even and in the supported range 2 <= layers[0] <= %d", nm, layers[0], kNcfMaxL0);
            for (int l = 1; l < n_layers; ++l)
                REQUIRE(layers[l] >= 1 && layers[l] <= kNcfMaxW, "%s: layers[%d] = %d is outside the supported range 1 <= width <= %d", nm, l,
                        layers[l], kNcfMaxW);
            REQUIRE(act >= 0 && act < NACT_COUNT, "%s: unknown activation %d", nm, act);
        }
        if (kind == NCF_NEUMF)
            REQUIRE(layers[n_layers - 1] == num_factors, "NeuMF: layers[-1] = %d must equal num_factors = %d", layers[n_layers - 1], num_factors);
        check_csr(nm, "the training matrix", n_users, n_items, indptr, indices, data, kCsrFiniteValues);
        const int64_t nnz = indptr[n_users];
        REQUIRE(nnz < (1ll << 31), "%s: %lld stored entries are more than the sampler's 2^31 - 1", nm, (long long)nnz);
        std::unique_ptr<cornac_hip_ncf> h(new cornac_hip_ncf());
        h->n_users = n_users; h->n_items = n_items; h->nnz = nnz;
        h->N.kind = kind;
        h->N.F = kind == NCF_MLP ? 0 : num_factors;
        h->N.nl = kind == NCF_GMF ? 0 : n_layers;
        h->N.act = kind == NCF_GMF ? 0 : act;
        for (int l = 0; l < h->N.nl; ++l) h->N.width[l] = layers[l];
        ncf_layout(h.get());
        std::vector<int32_t> ent_user((size_t)nnz), n_pos((size_t)n_users);
        for (int64_t u = 0; u < n_users; ++u) {
            int32_t c = 0;
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) {
                ent_user[(size_t)e] = (int32_t)u;
                c += data[e] > 0.0 ? 1 : 0;
            }
            n_pos[(size_t)u] = c;
            if (h->no_negative_user < 0 && indptr[u + 1] > indptr[u] && c == n_items) h->no_negative_user = u;
        }
        h->open(device);
        for (DevBuf<float> *b : {&h->w, &h->s1, &h->s2}) {
            alloc_named(*b, (size_t)h->total, nm, "the tables and the learner's state");
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        h->rows.upload(nm, "the training matrix", n_users, indptr, indices, data, h->stream);
        alloc_named(h->ent_user, (size_t)nnz, nm, "the entries' users");
        alloc_named(h->n_pos, (size_t)n_users, nm, "the users' positive counts");
        if (nnz) h->ent_user.upload(ent_user.data(), (size_t)nnz, h->stream);
        h->n_pos.upload(n_pos.data(), (size_t)n_users, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_ncf_destroy(cornac_hip_ncf_t h) { return destroy_handle(h); }

static const char *ncf_name(cornac_hip_ncf_t h) { return kNcfKindName[h->N.kind]; }

int cornac_hip_ncf_n_tables(cornac_hip_ncf_t h, int *n) {
    return guarded([&] {
        REQUIRE(h != nullptr && n != nullptr, "NCF handle / n is NULL");
        *n = h->all.n;
    });
}

int cornac_hip_ncf_set_params(cornac_hip_ncf_t h, const float *const *tables) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        REQUIRE(tables != nullptr, "%s: tables is NULL", ncf_name(h));
        put_tables(h->stream, h->w.p, h->slots, tables);
    });
}

int cornac_hip_ncf_get_params(cornac_hip_ncf_t h, float *const *tables) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        REQUIRE(tables != nullptr, "%s: tables is NULL", ncf_name(h));
        get_tables(h->stream, h->w.p, h->slots, tables);
    });
}

int cornac_hip_ncf_get_state(cornac_hip_ncf_t h, float *const *s1, float *const *s2, int64_t *t) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        if (s1) get_tables(h->stream, h->s1.p, h->slots, s1);
        if (s2) get_tables(h->stream, h->s2.p, h->slots, s2);
        if (t) *t = h->t;
    });
}

int cornac_hip_ncf_reset_optimizer(cornac_hip_ncf_t h) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        zero_state(h->stream, {&h->s1, &h->s2});
        h->t = 0;
    });
}

static void ncf_ensure_epoch(cornac_hip_ncf_t h, int64_t samples, int64_t steps) {
    const char *nm = ncf_name(h), *what = "an epoch's samples";
    if (samples > h->cap_samples) {
        for (DevBuf<int32_t> *b : {&h->users, &h->items, &h->order_u, &h->sorted_u, &h->order_i, &h->sorted_i})
            alloc_named(*b, (size_t)samples, nm, what);
        alloc_named(h->labels, (size_t)samples, nm, what);
        alloc_named(h->loss, (size_t)samples, nm, what);
        h->cap_samples = samples;
    }
    if (steps > h->cap_steps) {
        alloc_named(h->step_ptr, (size_t)steps + 1, nm, what);
        alloc_named(h->step_loss, (size_t)steps, nm, what);
        h->cap_steps = steps;
    }
}

static void ncf_ensure_step(cornac_hip_ncf_t h, int64_t n) {
    if (n <= h->cap_step) return;
    const char *nm = ncf_name(h), *what = "a step's activations and gradients";
    const size_t c = (size_t)n, sw = (size_t)std::max(h->N.sumw, 1), F = (size_t)std::max(h->N.F, 1);
    for (DevBuf<float> *b : {&h->hbuf, &h->dbuf, &h->gabuf}) alloc_named(*b, c * sw, nm, what);
    for (DevBuf<float> *b : {&h->hg, &h->gu, &h->gi}) alloc_named(*b, c * F, nm, what);
    alloc_named(h->dl, c, nm, what);
    h->cap_step = n;
}

static void ncf_check_opt(cornac_hip_ncf_t h, float lr, float reg, int learner) {
    REQUIRE(learner >= 0 && learner < NCF_LEARNERS, "%s: unknown learner %d", ncf_name(h), learner);
    REQUIRE(std::isfinite(lr) && std::isfinite(reg), "%s: lr and reg must be finite", ncf_name(h));
}

// the steps over the samples that lie on the device (h->users, items, labels, step_ptr); step_ptr is the host's copy
static void ncf_train(cornac_hip_ncf_t h, int64_t steps, const int64_t *step_ptr, float lr, float reg, int learner, double *loss_sum,
                      double *step_loss) {
    int64_t max_n = 0;
    for (int64_t s = 0; s < steps; ++s) max_n = std::max(max_n, step_ptr[s + 1] - step_ptr[s]);
    ncf_ensure_step(h, max_n);
    ncf_order_kernel<<<dim3((unsigned)steps, grid(max_n), 2), kVaeBlock, 0, h->stream>>>(
        h->step_ptr.p, h->users.p, h->items.p, h->order_u.p, h->sorted_u.p, h->order_i.p, h->sorted_i.p);
    HIP_CHECK(hipGetLastError());
    for (int64_t s = 0; s < steps; ++s) {
        const int64_t base = step_ptr[s], n = step_ptr[s + 1] - base;
        h->t += 1;
        NcfOpt opt{};
        opt.learner = learner; opt.lr = lr; opt.reg = reg;
        opt.adam = adam_at(h->t, lr);
        ncf_forward_kernel<true><<<grid(n, kNcfTile), kVaeBlock, 0, h->stream>>>(
            h->N, h->w.p, h->users.p + base, h->items.p + base, h->n_items, n, h->labels.p + base, 1.0f / (float)n, nullptr, h->hbuf.p,
            h->dbuf.p, h->gabuf.p, h->hg.p, h->gu.p, h->gi.p, h->dl.p, h->loss.p + base);
        ncf_sweep_kernel<<<grid(h->small_total, kNcfSlices) + grid(h->emb_total), kVaeBlock, 0, h->stream>>>(
            h->N, h->emb, h->emb_total, h->small, h->small_total, h->w.p, h->s1.p, h->s2.p, (int)n, h->order_u.p + base, h->sorted_u.p + base,
            h->order_i.p + base, h->sorted_i.p + base, h->hbuf.p, h->gabuf.p, h->hg.p, h->gu.p, h->gi.p, h->dl.p, opt);
        HIP_CHECK(hipGetLastError());
    }
    ncf_loss_kernel<<<(unsigned)steps, kVaeBlock, 0, h->stream>>>(h->step_ptr.p, h->loss.p, h->step_loss.p);
    HIP_CHECK(hipGetLastError());
    std::vector<double> losses((size_t)steps);
    h->step_loss.download(losses.data(), (size_t)steps, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    double total = 0.0;
    for (int64_t s = 0; s < steps; ++s) {
        if (step_loss) step_loss[s] = losses[(size_t)s];
        total += losses[(size_t)s];
    }
    if (loss_sum) *loss_sum = total;
}

int cornac_hip_ncf_fit_epoch(cornac_hip_ncf_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users, const int32_t *items,
                             const float *labels, float lr, float reg, int learner, double *loss_sum, double *step_loss) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        const char *nm = ncf_name(h);
        ncf_check_opt(h, lr, reg, learner);
        REQUIRE(steps >= 1 && steps < (1ll << 31), "%s: the number of steps must be in 1 .. 2^31 - 1", nm);
        REQUIRE(step_ptr && users && items && labels, "%s: step_ptr / users / items / labels are NULL", nm);
        REQUIRE(step_ptr[0] == 0, "%s: step_ptr does not start at 0", nm);
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t n = step_ptr[s + 1] - step_ptr[s];
            REQUIRE(n >= 1 && n <= kNcfMaxStep, "%s: step %lld has %lld samples, outside the supported range 1 <= batch_size * (1 + num_neg) <= %d",
                    nm, (long long)s, (long long)n, kNcfMaxStep);
        }
        const int64_t total = step_ptr[steps];
        for (int64_t q = 0; q < total; ++q) {
            REQUIRE(users[q] >= 0 && users[q] < h->n_users, "%s: user %d out of range", nm, users[q]);
            REQUIRE(items[q] >= 0 && items[q] < h->n_items, "%s: item %d out of range", nm, items[q]);
            REQUIRE(labels[q] >= 0.f && labels[q] <= 1.f, "%s: label %g of sample %lld is outside [0, 1]", nm, (double)labels[q], (long long)q);
        }
        ncf_ensure_epoch(h, total, steps);
        h->users.upload(users, (size_t)total, h->stream);
        h->items.upload(items, (size_t)total, h->stream);
        h->labels.upload(labels, (size_t)total, h->stream);
        h->step_ptr.upload(step_ptr, (size_t)steps + 1, h->stream);
        ncf_train(h, steps, step_ptr, lr, reg, learner, loss_sum, step_loss);
    });
}

// the epoch's samples drawn into h->users / items / labels / step_ptr; returns the host's step_ptr
static std::vector<int64_t> ncf_draw(cornac_hip_ncf_t h, int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch) {
    const char *nm = ncf_name(h);
    REQUIRE(num_neg >= 0 && batch_size >= 1 && batch_size * (1 + (int64_t)num_neg) <= kNcfMaxStep,
            "%s: batch_size = %lld with num_neg = %d is outside the supported range 1 <= batch_size * (1 + num_neg) <= %d", nm,
            (long long)batch_size, num_neg, kNcfMaxStep);
    REQUIRE(h->nnz >= 1, "%s: the training matrix has no stored entry to sample", nm);
    REQUIRE(num_neg == 0 || h->no_negative_user < 0,
            "%s: user %lld rates every item positively: there is no negative to draw for it (the reference would not return)", nm,
            (long long)h->no_negative_user);
    const int64_t per = 1 + num_neg, steps = (h->nnz + batch_size - 1) / batch_size, total = h->nnz * per;
    REQUIRE(steps < (1ll << 31), "%s: the number of steps must be below 2^31", nm);
    std::vector<int64_t> ptr((size_t)steps + 1);
    for (int64_t s = 0; s <= steps; ++s) ptr[(size_t)s] = std::min(s * batch_size, h->nnz) * per;
    ncf_ensure_epoch(h, total, steps);
    h->step_ptr.upload(ptr.data(), (size_t)steps + 1, h->stream);
    ncf_draw_kernel<<<grid(total), kVaeBlock, 0, h->stream>>>(h->rows.ptr.p, h->rows.idx.p, h->rows.val.p, h->ent_user.p, h->n_pos.p,
                                                              h->nnz, h->n_items, batch_size, num_neg, seed, epoch, h->users.p,
                                                              h->items.p, h->labels.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(h->stream));   // (ptr is the upload's source)
    return ptr;
}

int cornac_hip_ncf_draw_epoch(cornac_hip_ncf_t h, int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch, int64_t *step_ptr,
                              int32_t *users, int32_t *items, float *labels) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        REQUIRE(step_ptr && users && items && labels, "%s: step_ptr / users / items / labels are NULL", ncf_name(h));
        const std::vector<int64_t> ptr = ncf_draw(h, batch_size, num_neg, seed, epoch);
        const size_t total = (size_t)ptr.back();
        std::copy(ptr.begin(), ptr.end(), step_ptr);
        h->users.download(users, total, h->stream);
        h->items.download(items, total, h->stream);
        h->labels.download(labels, total, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ncf_fit_epoch_sampled(cornac_hip_ncf_t h, int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch, float lr, float reg,
                                     int learner, double *loss_sum, double *step_loss) {
    return guarded([&] {
        check_handle(h, "NCF handle");
        ncf_check_opt(h, lr, reg, learner);
        const std::vector<int64_t> ptr = ncf_draw(h, batch_size, num_neg, seed, epoch);
        ncf_train(h, (int64_t)ptr.size() - 1, ptr.data(), lr, reg, learner, loss_sum, step_loss);
    });
}

// users[0 .. n) in chunks: whole rows (items == NULL) or pairs; both through the forward kernel, sample by sample
static void ncf_predict(cornac_hip_ncf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    check_handle(h, "NCF handle");
    const char *nm = ncf_name(h);
    check_ids(nm, users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t I = h->n_items;
    const int64_t B = items ? std::min(n, kNcfScorePairs)
                            : std::min<int64_t>(n, std::max<int64_t>(1, std::min<int64_t>(kNcfScoreUsers, kNcfScoreBytes / (4 * I))));
    const int64_t width = items ? 1 : I;
    if (h->out.n < (size_t)(B * width)) alloc_named(h->out, (size_t)(B * width), nm, "the scores");
    for_each_chunk(nm, *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        ncf_forward_kernel<false><<<grid(nb * width, kNcfTile), kVaeBlock, 0, h->stream>>>(
            h->N, h->w.p, h->user_ids.p, items ? h->item_ids.p : nullptr, I, nb * width, nullptr, 0.f, h->out.p, nullptr, nullptr, nullptr,
            nullptr, nullptr, nullptr, nullptr, nullptr);
        h->out.download(out + b0 * width, (size_t)(nb * width), h->stream);
    });
}

int cornac_hip_ncf_score_users(cornac_hip_ncf_t h, const int32_t *users, int64_t n, float *out) {
    return guarded([&] { ncf_predict(h, users, nullptr, n, out); });
}

int cornac_hip_ncf_score_pairs(cornac_hip_ncf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "NCF: items is NULL");
        ncf_predict(h, users, items, n, out);
    });
}

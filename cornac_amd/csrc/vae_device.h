// Device code shared by the autoencoder models (vaecf.hip, bivae.hip, recvae.hip): the workgroup size, the activations with
// their derivatives, torch.optim.Adam's update of one entry, the workgroup's fixed-tree sum and maximum, the uniform and
// normal draws from Philox words, the register-tiled product with its three epilogues, Adam on a first layer's table and
// the gather of a score per pair.  ncf.hip and graph.h (lightgcn.hip, ngcf.hip) take the workgroup size and Adam's update
// from here, through vae_host.h.  The arithmetic is VAECF's and RecVAE's, and their tests hold it in place.
// The kernels sit in an unnamed namespace: every source that includes this header gets its own copies.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace chip {

constexpr int kVaeBlock = 256;
enum { ACT_TANH = 0, ACT_SIGMOID, ACT_RELU, ACT_RELU6, ACT_ELU, ACT_COUNT };

struct VaeAdam {
    float omb1, b2, omb2, step, bc2s, eps;
};

__device__ inline void vae_adam(float *w, float *m, float *v, int64_t idx, float g, const VaeAdam &a) {
    float mm = m[idx];
    mm = mm + (g - mm) * a.omb1;
    const float vv = v[idx] * a.b2 + a.omb2 * g * g;
    m[idx] = mm;
    v[idx] = vv;
    const float denom = sqrtf(vv) / a.bc2s + a.eps;
    w[idx] = w[idx] - a.step * (mm / denom);
}

__device__ inline float vae_act(int act, float x, float *d) {
    switch (act) {
    case ACT_TANH: { const float t = tanhf(x); *d = 1.f - t * t; return t; }
    case ACT_SIGMOID: { const float s = 1.f / (1.f + expf(-x)); *d = s * (1.f - s); return s; }
    case ACT_RELU: *d = x > 0.f ? 1.f : 0.f; return x > 0.f ? x : 0.f;
    case ACT_RELU6: *d = (x > 0.f && x < 6.f) ? 1.f : 0.f; return fminf(fmaxf(x, 0.f), 6.f);
    default:
        if (x > 0.f) { *d = 1.f; return x; }
        *d = expf(x);
        return expm1f(x);
    }
}

namespace {

constexpr int kVaeTile = 64, kVaeTk = 16;   // the product's output tile (square) and its step along k

// fixed tree over the workgroup's 256 values: the order of the sum is part of the results
__device__ inline float block_sum(float v, float *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = kVaeBlock / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

__device__ inline float block_max(float v, float *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = kVaeBlock / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = fmaxf(sh[t], sh[t + s]);
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// a Philox word's top 24 bits as the centre of their cell of (0, 1); Box-Muller's cosine branch of two words
__device__ inline float unit(uint32_t r) { return ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f); }
__device__ inline float normal(uint32_t r0, uint32_t r1) { return sqrtf(-2.f * logf(unit(r0))) * cosf(6.283185307179586f * unit(r1)); }

// ---- the product --------------------------------------------------------------------------------------------------------------
// sum_k A(m, k) B(k, n) for m < M, n < N over k in [z kchunk, (z + 1) kchunk) below K, ascending, z = blockIdx.z;
// A(m, k) = A[m a_sm + k a_sk] and B(k, n) = B[k b_sk + n b_sn]; AK / BK say that the operand is contiguous along k (the
// staging loads follow it).  blockIdx.x counts the 64 x 64 tiles of the output, rows of tiles first.  The output is dense,
// N floats to a row:
// EPI 0: C[m N + n] = acc (+ bias[n]) (+ add[m N + n]); bias and add may each be NULL, add may be C
//     1: C[(z M + m) N + n] = acc: the ranges' partial sums, one plane each
//     2: Adam on C / am / av [m N + n] with g = acc
template <bool AK, bool BK, int EPI>
__global__ __launch_bounds__(kVaeBlock) void vae_gemm_kernel(const float *__restrict__ A, int64_t a_sm, int64_t a_sk,
                                                             const float *__restrict__ B, int64_t b_sk, int64_t b_sn, int64_t M, int64_t N,
                                                             int64_t K, int64_t kchunk, float *C, const float *bias, const float *add,
                                                             float *am, float *av, VaeAdam ad) {
    __shared__ float sA[kVaeTk][kVaeTile + 4];
    __shared__ float sB[kVaeTk][kVaeTile + 4];
    const int64_t tiles_n = (N + kVaeTile - 1) / kVaeTile;
    const int64_t n0 = ((int64_t)blockIdx.x % tiles_n) * kVaeTile, m0 = ((int64_t)blockIdx.x / tiles_n) * kVaeTile;
    const int64_t k_begin = (int64_t)blockIdx.z * kchunk, k_end = K < k_begin + kchunk ? K : k_begin + kchunk;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += kVaeTk) {
#pragma unroll
        for (int q = 0; q < kVaeTile * kVaeTk / kVaeBlock; ++q) {
            const int idx = threadIdx.x + kVaeBlock * q;
            const int kk = AK ? idx % kVaeTk : idx / kVaeTile, mm = AK ? idx / kVaeTk : idx % kVaeTile;
            const int64_t gm = m0 + mm, gk = k0 + kk;
            sA[kk][mm] = (gm < M && gk < k_end) ? A[gm * a_sm + gk * a_sk] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kVaeTile * kVaeTk / kVaeBlock; ++q) {
            const int idx = threadIdx.x + kVaeBlock * q;
            const int kk = BK ? idx % kVaeTk : idx / kVaeTile, nn = BK ? idx / kVaeTk : idx % kVaeTile;
            const int64_t gn = n0 + nn, gk = k0 + kk;
            sB[kk][nn] = (gn < N && gk < k_end) ? B[gk * b_sk + gn * b_sn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kVaeTk; ++kk) {
            float a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = sA[kk][ty * 4 + q];
                b[q] = sB[kk][tx * 4 + q];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(a[p], b[q], acc[p][q]);
        }
        __syncthreads();
    }
    if (EPI == 0) {   // bias and add are tested once, outside the loops over the thread's 4 x 4 outputs
        const int64_t gm0 = m0 + ty * 4, gn0 = n0 + tx * 4;
        if (bias) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (gn0 + q >= N) continue;
                const float b = bias[gn0 + q];
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p][q] += b;
            }
        }
        if (add) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (gm0 + p < M && gn0 + q < N) acc[p][q] += add[(gm0 + p) * N + gn0 + q];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (gm0 + p < M && gn0 + q < N) C[(gm0 + p) * N + gn0 + q] = acc[p][q];
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t gm = m0 + ty * 4 + p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t gn = n0 + tx * 4 + q;
            if (gm >= M || gn >= N) continue;
            if (EPI == 1) {
                C[((int64_t)blockIdx.z * M + gm) * N + gn] = acc[p][q];
            } else {
                vae_adam(C, am, av, gm * N + gn, acc[p][q], ad);
            }
        }
    }
}

// ---- Adam on a first layer's table w / am / av [at ..), one row of h per column id n < N of the batch's rows -------------------
// The gradient of row n is the sum of ga1[b] over the batch's rows r0 .. r0 + nb that hold n: a range of n's ascending holder
// list (col_ptr, col_idx), found by bisection (batches are consecutive id ranges).  Rows that nobody of the batch holds get
// g = 0 and still decay and move.  One thread per entry.
__global__ void vae_w1_adam_kernel(float *w, float *am, float *av, int64_t at, int64_t N, int h, int64_t r0, int64_t nb,
                                   const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ col_idx,
                                   const float *__restrict__ ga1, VaeAdam ad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * h) return;
    const int64_t n = e / h, j = e % h;
    int64_t lo = col_ptr[n], hi = col_ptr[n + 1];
    const int64_t end = hi;
    while (lo < hi) {   // the first of n's holders that is not below r0
        const int64_t mid = (lo + hi) >> 1;
        if (col_idx[mid] < r0) lo = mid + 1; else hi = mid;
    }
    float g = 0.f;
    for (; lo < end && col_idx[lo] < r0 + nb; ++lo) g += ga1[((int64_t)col_idx[lo] - r0) * h + j];
    vae_adam(w, am, av, at + e, g, ad);
}

// out[q] = p[q, items[q]] of the rows p [n x I]
__global__ void gather_pairs_kernel(const float *__restrict__ p, int64_t I, const int32_t *__restrict__ items, int64_t n, float *out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = p[q * I + items[q]];
}

}  // namespace
}  // namespace chip

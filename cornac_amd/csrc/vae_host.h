// Host side of vae_device.h: torch.optim.Adam's coefficients at a step, the launch grids, the launchers of the tiled product
// (a Linear layer's forward, its backward in the input, Adam on its weight, the split-range partial sums).  Included by
// vaecf.hip, bivae.hip and recvae.hip; ncf.hip and graph.h (lightgcn.hip, ngcf.hip) take adam_at and grid.  Host code only; a
// refusal carries the model's prefix.
#pragma once
#include "sparse_model.h"
#include "vae_device.h"

namespace chip {
namespace {

// torch.optim.Adam (betas 0.9, 0.999, eps 1e-8) at step t >= 1.  torch holds the betas as doubles and rounds 1 - beta to
// float32 when the tensor operation takes it: 1.f - 0.999f is 1.3e-5 below (float)(1.0 - 0.999), which puts every early
// step 6.4e-6 off.  The bias corrections are doubles there too, and lr / bc1 is rounded once.
inline VaeAdam adam_at(int64_t t, float lr) {
    const double bc1 = 1.0 - std::pow(0.9, (double)t), bc2 = 1.0 - std::pow(0.999, (double)t);
    return VaeAdam{(float)(1.0 - 0.9), 0.999f, (float)(1.0 - 0.999), (float)((double)lr / bc1), (float)std::sqrt(bc2), 1e-8f};
}

inline unsigned grid(int64_t n, int64_t per = kVaeBlock) { return (unsigned)((n + per - 1) / per); }

// the 64 x 64 tiles of an M x N output
inline unsigned tiles(const char *model, int64_t M, int64_t N) {
    const int64_t t = ((M + kVaeTile - 1) / kVaeTile) * ((N + kVaeTile - 1) / kVaeTile);
    REQUIRE(t < (1ll << 31), "%s: %lld x %lld is more than a product's grid holds", model, (long long)M, (long long)N);
    return (unsigned)t;
}

// C[M x N] = A[M x K] W[N x K]^T (+ bias) (+ add): a Linear layer's forward
inline void linear(hipStream_t stream, const char *model, const float *A, const float *W, const float *bias, const float *add, int64_t M,
                   int64_t N, int64_t K, float *C) {
    vae_gemm_kernel<true, true, 0><<<dim3(tiles(model, M, N)), kVaeBlock, 0, stream>>>(A, K, 1, W, 1, K, M, N, K, K + kVaeTk, C, bias, add,
                                                                                      nullptr, nullptr, VaeAdam{});
}

// C[M x N] = A[M x K] W[K x N] (+ add): a Linear layer's backward in its input
inline void linear_back(hipStream_t stream, const char *model, const float *A, const float *W, const float *add, int64_t M, int64_t N,
                        int64_t K, float *C) {
    vae_gemm_kernel<true, false, 0><<<dim3(tiles(model, M, N)), kVaeBlock, 0, stream>>>(A, K, 1, W, N, 1, M, N, K, K + kVaeTk, C, nullptr, add,
                                                                                       nullptr, nullptr, VaeAdam{});
}

// part[s, M x N] = A[M x K] W[K x N] over the s-th of n_split ranges of kchunk along K: linear_back's sum in fixed pieces,
// which the caller adds in ascending range order
inline void linear_back_split(hipStream_t stream, const char *model, const float *A, const float *W, int64_t M, int64_t N, int64_t K,
                              int64_t kchunk, int n_split, float *part) {
    vae_gemm_kernel<true, false, 1><<<dim3(tiles(model, M, N), 1, (unsigned)n_split), kVaeBlock, 0, stream>>>(
        A, K, 1, W, N, 1, M, N, K, kchunk, part, nullptr, nullptr, nullptr, nullptr, VaeAdam{});
}

// Adam on w / m / v [N x K] with g = Gy[nb x N]^T X[nb x K], each tile applied at once: no gradient table
inline void weight_adam(hipStream_t stream, const char *model, const float *Gy, const float *X, int64_t nb, int64_t N, int64_t K, float *w,
                        float *m, float *v, const VaeAdam &ad) {
    vae_gemm_kernel<false, false, 2><<<dim3(tiles(model, N, K)), kVaeBlock, 0, stream>>>(Gy, 1, N, X, K, 1, N, K, nb, nb + kVaeTk, w, nullptr,
                                                                                        nullptr, m, v, ad);
}

}  // namespace
}  // namespace chip

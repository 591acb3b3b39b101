// Device helpers shared by the two autoencoder models (vaecf.hip, bivae.hip): the workgroup size, the activations with
// their derivatives, and torch.optim.Adam's update of one entry.  Moved here from vaecf.hip as they stood: their arithmetic
// is VAECF's, and its tests hold it in place.
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

}  // namespace chip

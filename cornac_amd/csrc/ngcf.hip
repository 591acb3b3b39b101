// NGCF (Wang et al. 2019; cornac/models/ngcf/ngcf.py:14-185, recom_ngcf.py:137-199) on gfx950, float32 throughout.  The
// handle owns LightGCN's normalised adjacency A (graph.h: one CSR over users then items, float32 weights (deg deg)^-1/2), the
// rows' weight sums c_r, ONE parameter buffer [X_0 = user table | item table ; per layer W1, b1, W2, b2] (every piece starts
// at a multiple of four floats; the padding stays zero), Adam's two buffers of the same layout and its step counter, and
// per layer the activations that the backward pass reads.
//
// The reference computes two Linears per EDGE; the self loop and both edge types collapse to dense work per NODE.  Layer l,
// input X [N x d_in], output [N x d_out]:
//     s = A X                                                              hop (graph.h), whose epilogue also writes
//     P1 = X + s,  P2 = s * X                                              the two GEMM operands
//     z = P1 W1^T + P2 W2^T + b1 + c (b1 + b2)                             gemm_block (fp32 MFMA), one 128 x 128 block per workgroup
//     a = dropout_p(leaky_relu(z, 0.2)),  y = a / max(|a|_2 per row, 1e-12)  in the GEMM's epilogue where d_out <= 128 (a row's
//                                                                          columns sit in one workgroup), else a second pass
// E = [X_0 | X_1 | .. | X_L], width D; the BPR loss and the gradient rows at E are LightGCN's kernels at width D.  Backward, per
// layer from the top, gy = E's gradient slice + what the layer above sent:
//     ga = (gy - y (y . gy)) / |a|   (gy / 1e-12 for a row below 1e-12, as torch's clamp does)
//     gz = ga * mask / (1 - p) * (z > 0 ? 1 : 0.2)                         one wave per row
//     gW1 = gz^T P1, gW2 = gz^T P2, gb1 = sum_r (1 + c_r) gz_r, gb2 = sum_r c_r gz_r
//                                                                          per chunk of kNgcfWgradRows rows (MFMA for the weights);
//                                                                          the chunks' partials are added in chunk order
//     q1 = gz W1, q2 = gz W2;  T = q1 + q2 * X,  R = q1 + q2 * s           one GEMM kernel, two accumulators
//     gX = R + A T                                                         the same hop (A is symmetric)
// then torch's Adam over the whole parameter buffer, densely: every row feeds the weights, so nothing is skipped.
//
// THE DROPOUT MASK is a pure function of (key, Adam step t, layer, row, column) through rng.h's Philox4x32-10: with
// e = row * d_out + column, the counter is (low word of e / 4, high word of e / 4, layer, t mod 2^32), the key the two
// halves of the model's 64-bit dropout key (low, high), and entry e is KEPT iff output word (e mod 4) >= floor(p * 2^32 + 0.5)
// (p as the float32 it was given, capped at 2^32 - 1).  A kept entry is multiplied by the float32 quotient 1 / (1 - p); a
// layer with p = 0 draws nothing and multiplies nothing; `propagate` is eval mode and applies no dropout.
// tests/ngcf_cases.py restates this in numpy.
//
// No atomics; every sum has one fixed order, so the same inputs give the same bits.
#include "graph.h"
#include "mfma_gemm.h"
#include "rng.h"

namespace chip {
namespace {

constexpr int kNgcfWgradRows = 2048;   // rows of one chunk of the weight and bias gradients (_lib.NgcfModel.WGRAD_ROWS)
constexpr float kNgcfEps = 1e-12f;     // F.normalize's eps
constexpr float kNgcfSlope = 0.2f;     // nn.LeakyReLU(0.2)

struct NgcfDrop {
    uint32_t k0, k1, layer, t, thresh;
    float keep;
    int on;
};

__device__ inline bool ngcf_kept(const NgcfDrop &dr, int64_t row, int dout, int col) {
    const uint64_t e = (uint64_t)row * (uint64_t)dout + (uint64_t)col, ctr = e >> 2;
    uint32_t o[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), dr.layer, dr.t, dr.k0, dr.k1, o);
    const int q = (int)(e & 3);
    const uint32_t word = q == 0 ? o[0] : q == 1 ? o[1] : q == 2 ? o[2] : o[3];
    return word >= dr.thresh;
}

__device__ inline float ngcf_act(float z, const NgcfDrop &dr, int64_t row, int dout, int col) {
    float a = z > 0.f ? z : z * kNgcfSlope;
    if (dr.on) a = ngcf_kept(dr, row, dout, col) ? a * dr.keep : 0.f;
    return a;
}

// ---- the hops' epilogues ---------------------------------------------------------------------------------------------------------------
struct NgcfFwd {   // s = A X: keeps s and writes the GEMM's operands
    const float *X;
    float *S, *P1, *P2;
    template <int VEC>
    __device__ inline void finish(int64_t row, int c, int d, const LgcnVec<VEC> &h) const {
        const int64_t at = row * d + c;
        const LgcnVec<VEC> x = lgcn_load<VEC>(X + at);
        LgcnVec<VEC> p1, p2;
#pragma unroll
        for (int q = 0; q < VEC; ++q) { p1.v[q] = x.v[q] + h.v[q]; p2.v[q] = h.v[q] * x.v[q]; }
        lgcn_store<VEC>(S + at, h);
        lgcn_store<VEC>(P1 + at, p1);
        lgcn_store<VEC>(P2 + at, p2);
    }
};

struct NgcfBwd {   // gX = R + A T (+ E's gradient slice, for the tables: ge [N x D] at column off)
    const float *R, *ge;
    int D, off;
    float *out;
    template <int VEC>
    __device__ inline void finish(int64_t row, int c, int d, const LgcnVec<VEC> &h) const {
        const int64_t at = row * d + c;
        LgcnVec<VEC> r = lgcn_load<VEC>(R + at);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            r.v[q] = r.v[q] + h.v[q];
            if (ge) r.v[q] = ge[row * D + off + c + q] + r.v[q];   // (scalar: the slice's first column is any)
        }
        lgcn_store<VEC>(out + at, r);
    }
};

// E[:, 0 .. d0) = X_0
__global__ __launch_bounds__(kLgcnBlock) void ngcf_copy0_kernel(const float *__restrict__ X0, int64_t total, int d0, int D, float *E) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) E[(e / d0) * D + e % d0] = X0[e];
}

// ---- z = P1 W1^T + P2 W2^T + b1 + c (b1 + b2), one 128 x 128 block per workgroup; FUSED (d_out <= 128, gridDim.y = 1): the
// activation, the dropout and the row norm in the epilogue -------------------------------------------------------------------------------
template <bool FUSED>
__global__ __launch_bounds__(kWb) void ngcf_dense_kernel(const float *__restrict__ P1, const float *__restrict__ P2, const float *__restrict__ W1,
                                                         const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2,
                                                         const float *__restrict__ crow, int64_t N, int din, int dout, float *Z, float *Y,
                                                         float *nrm, float *E, int D, int off, NgcfDrop dr) {
    __shared__ GemmSmem sm;
    __shared__ float rs[2][kBM];
    const int64_t m0 = (int64_t)blockIdx.x * kBM, n0 = (int64_t)blockIdx.y * kBN;
    f32x16 acc[2][2];
    gemm_block<true, false>(P1, din, 1, W1, 1, din, N, dout, m0, n0, 0, din, sm, acc);
    gemm_block<true, false, false>(P2, din, 1, W2, 1, din, N, dout, m0, n0, 0, din, sm, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = (int)n0 + wn * 64 + j * 32 + l31;
        const float bb1 = col < dout ? b1[col] : 0.f, bb12 = col < dout ? b1[col] + b2[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float a = 0.f;
                if (row < N && col < dout) {
                    const float z = acc[i][j][r] + (bb1 + crow[row] * bb12);
                    Z[row * dout + col] = z;
                    if (FUSED) a = ngcf_act(z, dr, row, dout, col);
                }
                acc[i][j][r] = a;
            }
    }
    if (!FUSED) return;
    // a row's squared sum: its two 32-column blocks in the thread, 32 lanes by a butterfly, the two column waves through LDS
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float ss = acc[i][0][r] * acc[i][0][r] + acc[i][1][r] * acc[i][1][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) ss = ss + __shfl_xor(ss, o, 64);
            if (l31 == 0) rs[wn][wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] = ss;
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int64_t row = m0 + rl;
            if (row >= N) continue;
            const float n = sqrtf(rs[0][rl] + rs[1][rl]), den = fmaxf(n, kNgcfEps);
            if (wn == 0 && l31 == 0) nrm[row] = n;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = wn * 64 + j * 32 + l31;
                if (col >= dout) continue;
                const float y = acc[i][j][r] / den;
                Y[row * dout + col] = y;
                E[row * D + off + col] = y;
            }
        }
}

// the second pass for d_out > 128: one wave per row (d_out <= 256: four columns per lane)
__global__ __launch_bounds__(kLgcnBlock) void ngcf_act_kernel(const float *__restrict__ Z, int64_t N, int dout, float *Y, float *nrm, float *E, int D,
                                                              int off, NgcfDrop dr) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kLgcnBlock / 64) + (int)threadIdx.x / 64;
    if (row >= N) return;
    float a[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        a[k] = c < dout ? ngcf_act(Z[row * dout + c], dr, row, dout, c) : 0.f;
        ss = ss + a[k] * a[k];
    }
    const float n = sqrtf(lgcn_wave_sum(ss)), den = fmaxf(n, kNgcfEps);
    if (lane == 0) nrm[row] = n;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c >= dout) continue;
        const float y = a[k] / den;
        Y[row * dout + c] = y;
        E[row * D + off + c] = y;
    }
}

// ---- gz: back through the row norm, the dropout and the LeakyReLU; one wave per row ----------------------------------------------------
// gy = ge[:, off ..) + gin (gin: what the layer above sent, NULL for the top layer)
__global__ __launch_bounds__(kLgcnBlock) void ngcf_gz_kernel(const float *__restrict__ Y, const float *__restrict__ Z, const float *__restrict__ nrm,
                                                             const float *__restrict__ ge, int D, int off, const float *__restrict__ gin, int64_t N,
                                                             int dout, float *GZ, NgcfDrop dr) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kLgcnBlock / 64) + (int)threadIdx.x / 64;
    if (row >= N) return;
    float gy[4], y[4], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        gy[k] = 0.f; y[k] = 0.f;
        if (c < dout) {
            gy[k] = ge[row * D + off + c];
            if (gin) gy[k] = gy[k] + gin[row * dout + c];
            y[k] = Y[row * dout + c];
        }
        dot = dot + y[k] * gy[k];
    }
    dot = lgcn_wave_sum(dot);
    const float n = nrm[row];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        if (c >= dout) continue;
        const float ga = n < kNgcfEps ? gy[k] / kNgcfEps : (gy[k] - y[k] * dot) / n;
        float f = Z[row * dout + c] > 0.f ? 1.f : kNgcfSlope;
        if (dr.on) f = ngcf_kept(dr, row, dout, c) ? f * dr.keep : 0.f;
        GZ[row * dout + c] = ga * f;
    }
}

// ---- the weights' gradients of one chunk of rows: block (chunk, 128 x 128 tile, W1 or W2) ------------------------------------------------
__global__ __launch_bounds__(kWb) void ngcf_wgrad_kernel(const float *__restrict__ GZ, const float *__restrict__ P1, const float *__restrict__ P2,
                                                         int64_t N, int din, int dout, float *part, int64_t seg, int64_t rW1, int64_t rW2) {
    __shared__ GemmSmem sm;
    const int tiles_i = (din + kBN - 1) / kBN;
    const int64_t m0 = (int64_t)((int)blockIdx.y / tiles_i) * kBM, n0 = (int64_t)((int)blockIdx.y % tiles_i) * kBN;
    const int64_t r0 = (int64_t)blockIdx.x * kNgcfWgradRows, r1 = r0 + kNgcfWgradRows < N ? r0 + kNgcfWgradRows : N;
    f32x16 acc[2][2];
    gemm_block<false, true>(GZ, 1, dout, blockIdx.z ? P2 : P1, din, 1, dout, din, m0, n0, r0, r1, sm, acc);
    float *out = part + (int64_t)blockIdx.x * seg + (blockIdx.z ? rW2 : rW1);
    for_each_acc(acc, m0, n0, [&](int64_t row, int64_t col, float v) {
        if (row < dout && col < din) out[row * din + col] = v;
    });
}

// the biases' gradients of one chunk: the workgroup's 256 threads are R = 256 / d_out walkers per column; walker w of column o
// sums the chunk's rows r0 + w, r0 + w + R, .. ascending, and the column's walkers are then added in walker order
__global__ __launch_bounds__(kLgcnBlock) void ngcf_bgrad_kernel(const float *__restrict__ GZ, const float *__restrict__ crow, int64_t N, int dout,
                                                                float *part, int64_t seg, int64_t rb1, int64_t rb2) {
    __shared__ float sh1[kLgcnBlock], sh2[kLgcnBlock];
    const int R = kLgcnBlock / dout, tid = (int)threadIdx.x;   // (d_out <= 256: R >= 1)
    const int o = tid % dout, w = tid / dout;
    const int64_t r0 = (int64_t)blockIdx.x * kNgcfWgradRows, r1 = r0 + kNgcfWgradRows < N ? r0 + kNgcfWgradRows : N;
    float s1 = 0.f, s2 = 0.f;
    if (w < R) {
#pragma unroll 4
        for (int64_t r = r0 + w; r < r1; r += R) {
            const float g = GZ[r * dout + o], cg = crow[r] * g;
            s1 = s1 + (g + cg);
            s2 = s2 + cg;
        }
    }
    sh1[tid] = s1;
    sh2[tid] = s2;
    __syncthreads();
    if (w != 0) return;
    for (int k = 1; k < R; ++k) { s1 = s1 + sh1[k * dout + o]; s2 = s2 + sh2[k * dout + o]; }
    float *out = part + (int64_t)blockIdx.x * seg;
    out[rb1 + o] = s1;
    out[rb2 + o] = s2;
}

// the chunks' partials added in chunk order into the layer's piece of the gradient buffer
__global__ __launch_bounds__(kLgcnBlock) void ngcf_wreduce_kernel(const float *__restrict__ part, int64_t seg, int64_t chunks, float *grad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= seg) return;
    float s = part[e];
    for (int64_t k = 1; k < chunks; ++k) s = s + part[k * seg + e];
    grad[e] = s;
}

// ---- q1 = gz W1, q2 = gz W2;  T = q1 + q2 * X,  R = q1 + q2 * s ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWb) void ngcf_back_kernel(const float *__restrict__ GZ, const float *__restrict__ W1, const float *__restrict__ W2,
                                                        const float *__restrict__ X, const float *__restrict__ S, int64_t N, int din, int dout,
                                                        float *T, float *R) {
    __shared__ GemmSmem sm;
    const int64_t m0 = (int64_t)blockIdx.x * kBM, n0 = (int64_t)blockIdx.y * kBN;
    f32x16 q1[2][2], q2[2][2];
    gemm_block<true, true>(GZ, dout, 1, W1, din, 1, N, din, m0, n0, 0, dout, sm, q1);
    gemm_block<true, true>(GZ, dout, 1, W2, din, 1, N, din, m0, n0, 0, dout, sm, q2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int64_t col = n0 + wn * 64 + j * 32 + l31;
                if (row >= N || col >= din) continue;
                const int64_t at = row * din + col;
                T[at] = q1[i][j][r] + q2[i][j][r] * X[at];
                R[at] = q1[i][j][r] + q2[i][j][r] * S[at];
            }
}

struct NgcfLayer {
    int din = 0, dout = 0, off = 0;          // off: the output's first column in E
    int64_t oW1 = 0, ob1 = 0, oW2 = 0, ob2 = 0, seg = 0;   // places in the parameter buffer; the layer's piece is [oW1, oW1 + seg)
    float p = 0.f, keep = 1.f;
    uint32_t thresh = 0;
    DevBuf<float> S, P1, P2, Z, Y, nrm;
};

inline int64_t ngcf_up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_ngcf : ModelHandle {
    LgcnGraphDev g;
    int64_t n_users = 0, n_items = 0, N = 0, n_params = 0, chunks = 0, max_seg = 0;
    int d0 = 0, L = 0, D = 0, max_d = 0;
    uint64_t key = 0;
    int64_t t = 0;   // Adam's step counter
    std::unique_ptr<NgcfLayer[]> layers;   // [L] (the buffers do not move)
    DevBuf<float> crow;              // the rows' weight sums
    DevBuf<float> w, m, v, grad;     // the parameter buffer, Adam's state, the gradient
    std::vector<TableSlot> slots;    // the two tables and each layer's W1, b1, W2, b2 in w / m / v
    DevBuf<float> E, GE;             // [N x D]: the concatenated embeddings and the gradient at them
    DevBuf<float> GZ, T, R, gya, gyb;   // [N x max_d]: backward scratch
    DevBuf<float> wpart;             // [chunks x max_seg]: the weight and bias gradients' partials
    LgcnEpoch ep;
};

static NgcfDrop ngcf_drop(cornac_hip_ngcf_t h, int l, bool train) {
    const NgcfLayer &y = h->layers[(size_t)l];
    return NgcfDrop{(uint32_t)h->key, (uint32_t)(h->key >> 32), (uint32_t)l, (uint32_t)h->t, y.thresh, y.keep, train && y.p > 0.f ? 1 : 0};
}

static const float *ngcf_input(cornac_hip_ngcf_t h, int l) { return l == 0 ? h->w.p : h->layers[(size_t)l - 1].Y.p; }

// E from the parameters; train: with the dropout of Adam step h->t
static void ngcf_forward(cornac_hip_ngcf_t h, bool train) {
    const int64_t N = h->N;
    ngcf_copy0_kernel<<<grid(N * h->d0), kLgcnBlock, 0, h->stream>>>(h->w.p, N * h->d0, h->d0, h->D, h->E.p);
    for (int l = 0; l < h->L; ++l) {
        NgcfLayer &y = h->layers[(size_t)l];
        const float *X = ngcf_input(h, l), *w = h->w.p;
        lgcn_hop(h->g, y.din, X, NgcfFwd{X, y.S.p, y.P1.p, y.P2.p}, h->stream);
        const NgcfDrop dr = ngcf_drop(h, l, train);
        const unsigned rows = grid(N, kBM);
        if (y.dout <= kBN) {
            ngcf_dense_kernel<true><<<dim3(rows, 1), kWb, 0, h->stream>>>(y.P1.p, y.P2.p, w + y.oW1, w + y.ob1, w + y.oW2, w + y.ob2, h->crow.p, N,
                                                                         y.din, y.dout, y.Z.p, y.Y.p, y.nrm.p, h->E.p, h->D, y.off, dr);
        } else {
            ngcf_dense_kernel<false><<<dim3(rows, grid(y.dout, kBN)), kWb, 0, h->stream>>>(
                y.P1.p, y.P2.p, w + y.oW1, w + y.ob1, w + y.oW2, w + y.ob2, h->crow.p, N, y.din, y.dout, y.Z.p, y.Y.p, y.nrm.p, h->E.p, h->D,
                y.off, dr);
            ngcf_act_kernel<<<grid(N, kLgcnBlock / 64), kLgcnBlock, 0, h->stream>>>(y.Z.p, N, y.dout, y.Y.p, y.nrm.p, h->E.p, h->D, y.off, dr);
        }
        HIP_CHECK(hipGetLastError());
    }
}

// grad from GE (the gradient at E), over the activations that ngcf_forward(h, true) left
static void ngcf_backward(cornac_hip_ngcf_t h) {
    const int64_t N = h->N;
    const float *gin = nullptr;
    for (int l = h->L - 1; l >= 0; --l) {
        NgcfLayer &y = h->layers[(size_t)l];
        const float *w = h->w.p;
        ngcf_gz_kernel<<<grid(N, kLgcnBlock / 64), kLgcnBlock, 0, h->stream>>>(y.Y.p, y.Z.p, y.nrm.p, h->GE.p, h->D, y.off, gin, N, y.dout,
                                                                               h->GZ.p, ngcf_drop(h, l, true));
        const unsigned tiles = grid(y.dout, kBM) * grid(y.din, kBN);
        ngcf_wgrad_kernel<<<dim3((unsigned)h->chunks, tiles, 2), kWb, 0, h->stream>>>(h->GZ.p, y.P1.p, y.P2.p, N, y.din, y.dout, h->wpart.p, y.seg,
                                                                                     0, y.oW2 - y.oW1);
        ngcf_bgrad_kernel<<<(unsigned)h->chunks, kLgcnBlock, 0, h->stream>>>(h->GZ.p, h->crow.p, N, y.dout, h->wpart.p, y.seg, y.ob1 - y.oW1,
                                                                            y.ob2 - y.oW1);
        ngcf_wreduce_kernel<<<grid(y.seg), kLgcnBlock, 0, h->stream>>>(h->wpart.p, y.seg, h->chunks, h->grad.p + y.oW1);
        ngcf_back_kernel<<<dim3(grid(N, kBM), grid(y.din, kBN)), kWb, 0, h->stream>>>(h->GZ.p, w + y.oW1, w + y.oW2, ngcf_input(h, l),
                                                                                      y.S.p, N, y.din, y.dout, h->T.p, h->R.p);
        HIP_CHECK(hipGetLastError());
        float *out = l == 0 ? h->grad.p : (gin == h->gya.p ? h->gyb.p : h->gya.p);
        lgcn_hop(h->g, y.din, h->T.p, NgcfBwd{h->R.p, l == 0 ? h->GE.p : nullptr, h->D, 0, out}, h->stream);
        gin = out;
    }
}

int cornac_hip_ngcf_create(cornac_hip_ngcf_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, int emb_size, int num_layers, const int32_t *layer_sizes, const float *dropout_rates,
                           uint64_t dropout_key) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "ngcf: sizes must be positive");
        REQUIRE(n_users + n_items < (1ll << 31), "ngcf: n_users + n_items must be below 2^31");
        REQUIRE(emb_size >= 1 && emb_size <= kLgcnMaxD, "ngcf: emb_size = %d is outside the supported range 1 <= emb_size <= %d", emb_size,
                kLgcnMaxD);
        REQUIRE(num_layers >= 1 && num_layers <= kLgcnMaxLayers, "ngcf: num_layers = %d is outside the supported range 1 <= num_layers <= %d",
                num_layers, kLgcnMaxLayers);
        REQUIRE(layer_sizes && dropout_rates, "ngcf: layer_sizes / dropout_rates are NULL");
        for (int l = 0; l < num_layers; ++l) {
            REQUIRE(layer_sizes[l] >= 1 && layer_sizes[l] <= kLgcnMaxD, "ngcf: layer size %d = %d is outside the supported range 1 <= size <= %d", l,
                    layer_sizes[l], kLgcnMaxD);
            REQUIRE(dropout_rates[l] >= 0.f && dropout_rates[l] < 1.f, "ngcf: dropout rate %d = %g is outside the supported range 0 <= p < 1", l,
                    (double)dropout_rates[l]);
        }
        std::unique_ptr<cornac_hip_ngcf> h(new cornac_hip_ngcf());
        const char *nm = "ngcf";
        h->g.build(nm, n_users, n_items, indptr, indices);
        h->n_users = n_users; h->n_items = n_items;
        const int64_t N = h->N = h->g.n_nodes;
        h->d0 = emb_size; h->L = num_layers; h->key = dropout_key;
        h->layers.reset(new NgcfLayer[(size_t)num_layers]);
        int64_t at = ngcf_up4(N * emb_size);
        int din = emb_size, off = emb_size;
        h->max_d = emb_size;
        for (int l = 0; l < num_layers; ++l) {
            NgcfLayer &y = h->layers[(size_t)l];
            y.din = din; y.dout = layer_sizes[l]; y.off = off;
            y.oW1 = at;
            y.ob1 = y.oW1 + ngcf_up4((int64_t)y.dout * y.din);
            y.oW2 = y.ob1 + ngcf_up4(y.dout);
            y.ob2 = y.oW2 + ngcf_up4((int64_t)y.dout * y.din);
            at = y.ob2 + ngcf_up4(y.dout);
            y.seg = at - y.oW1;
            y.p = dropout_rates[l];
            y.keep = 1.f / (1.f - y.p);
            const double th = std::floor((double)y.p * 4294967296.0 + 0.5);
            y.thresh = (uint32_t)std::min(th, 4294967295.0);
            h->max_seg = std::max(h->max_seg, y.seg);
            h->max_d = std::max(h->max_d, y.dout);
            din = y.dout; off += y.dout;
        }
        h->D = off;
        h->n_params = at;
        h->slots = {{0, n_users, emb_size, false}, {n_users * emb_size, n_items, emb_size, false}};
        for (int l = 0; l < num_layers; ++l) {
            const NgcfLayer &y = h->layers[(size_t)l];
            h->slots.insert(h->slots.end(), {{y.oW1, y.dout, y.din, false}, {y.ob1, 1, y.dout, false},
                                             {y.oW2, y.dout, y.din, false}, {y.ob2, 1, y.dout, false}});
        }
        h->chunks = (N + kNgcfWgradRows - 1) / kNgcfWgradRows;
        const std::vector<float> crow = h->g.row_sums();
        h->open(device);
        h->g.upload(nm, h->max_d, h->stream);
        alloc_named(h->crow, (size_t)N, nm, "the rows' weight sums");
        h->crow.upload(crow.data(), (size_t)N, h->stream);
        const char *what = "the parameters, Adam's state and the gradient";
        for (DevBuf<float> *b : {&h->w, &h->m, &h->v, &h->grad}) {
            alloc_named(*b, (size_t)h->n_params, nm, what);
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        what = "the layers' activations";
        for (int l = 0; l < num_layers; ++l) {
            NgcfLayer &y = h->layers[(size_t)l];
            for (DevBuf<float> *b : {&y.S, &y.P1, &y.P2}) alloc_named(*b, (size_t)(N * y.din), nm, what);
            for (DevBuf<float> *b : {&y.Z, &y.Y}) alloc_named(*b, (size_t)(N * y.dout), nm, what);
            alloc_named(y.nrm, (size_t)N, nm, what);
        }
        for (DevBuf<float> *b : {&h->E, &h->GE}) alloc_named(*b, (size_t)(N * h->D), nm, "the concatenated embeddings and their gradient");
        for (DevBuf<float> *b : {&h->GZ, &h->T, &h->R, &h->gya, &h->gyb}) alloc_named(*b, (size_t)(N * h->max_d), nm, "the backward pass");
        alloc_named(h->wpart, (size_t)(h->chunks * h->max_seg), nm, "the weight gradients' partial sums");
        HIP_CHECK(hipMemsetAsync(h->wpart.p, 0, h->wpart.n * sizeof(float), h->stream));   // (the pieces' padding is never written)
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->g.drop_host();
        *out = h.release();
    });
}

int cornac_hip_ngcf_destroy(cornac_hip_ngcf_t h) { return destroy_handle(h); }

// the exported calls' user, item and layers [4 L] (a NULL array skips every layer) as one pointer list in the slots' order
template <class T>
static std::vector<T *> ngcf_list(cornac_hip_ngcf_t h, T *user, T *item, T *const *layers) {
    std::vector<T *> p(h->slots.size(), nullptr);
    p[0] = user;
    p[1] = item;
    if (layers) std::copy(layers, layers + 4 * h->L, p.begin() + 2);
    return p;
}

int cornac_hip_ngcf_set_params(cornac_hip_ngcf_t h, const float *user, const float *item, const float *const *layers) {
    return guarded([&] {
        check_handle(h, "ngcf handle");
        put_tables(h->stream, h->w.p, h->slots, ngcf_list(h, user, item, layers).data());
    });
}

int cornac_hip_ngcf_get_params(cornac_hip_ngcf_t h, float *user, float *item, float *const *layers) {
    return guarded([&] {
        check_handle(h, "ngcf handle");
        get_tables(h->stream, h->w.p, h->slots, ngcf_list(h, user, item, layers).data());
    });
}

int cornac_hip_ngcf_get_state(cornac_hip_ngcf_t h, float *m_user, float *m_item, float *const *m_layers, float *v_user, float *v_item,
                              float *const *v_layers, int64_t *t) {
    return guarded([&] {
        check_handle(h, "ngcf handle");
        get_tables(h->stream, h->m.p, h->slots, ngcf_list(h, m_user, m_item, m_layers).data());
        get_tables(h->stream, h->v.p, h->slots, ngcf_list(h, v_user, v_item, v_layers).data());
        if (t) *t = h->t;
    });
}

int cornac_hip_ngcf_reset_optimizer(cornac_hip_ngcf_t h) {
    return guarded([&] {
        check_handle(h, "ngcf handle");
        zero_state(h->stream, {&h->m, &h->v});
        h->t = 0;
    });
}

int cornac_hip_ngcf_propagate(cornac_hip_ngcf_t h, float *user_out, float *item_out) {
    return guarded([&] {
        check_handle(h, "ngcf handle");
        ngcf_forward(h, false);
        const size_t nu = (size_t)(h->n_users * h->D), ni = (size_t)(h->n_items * h->D);
        if (user_out) HIP_CHECK(hipMemcpyAsync(user_out, h->E.p, nu * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (item_out) HIP_CHECK(hipMemcpyAsync(item_out, h->E.p + nu, ni * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ngcf_fit_epoch(cornac_hip_ngcf_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users, const int32_t *pos,
                              const int32_t *neg, float lr, float lambda_reg, double *loss_out, double *bpr_out, double *reg_out) {
    return guarded([&] {
        // (the steps' shape is checked before the handle: it needs no device)
        const int64_t max_n = LgcnEpoch::check_steps("ngcf", steps, step_ptr);
        check_handle(h, "ngcf handle");
        REQUIRE(users && pos && neg, "ngcf: users / pos / neg are NULL");
        REQUIRE(std::isfinite(lr) && std::isfinite(lambda_reg), "ngcf: lr and lambda_reg must be finite");
        h->ep.stage("ngcf", h->n_users, h->n_items, steps, max_n, step_ptr, users, pos, neg, h->stream);
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t base = step_ptr[s], n = step_ptr[s + 1] - base;
            h->t += 1;
            ngcf_forward(h, true);
            h->ep.loss_and_gradient(h->E.p, h->D, h->n_users, h->N, base, n, lambda_reg, h->GE.p, h->stream);
            ngcf_backward(h);
            lgcn_adam_kernel<<<grid(h->n_params), kLgcnBlock, 0, h->stream>>>(h->w.p, h->m.p, h->v.p, h->grad.p, h->n_params,
                                                                              adam_at(h->t, lr));
            HIP_CHECK(hipGetLastError());
        }
        h->ep.losses(steps, (double)lambda_reg, loss_out, bpr_out, reg_out, h->stream);
    });
}

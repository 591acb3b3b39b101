// LightGCN (He et al. 2020; cornac/models/lightgcn/lightgcn.py:13-134, recom_lightgcn.py:143-189) on gfx950, float32
// throughout.  The handle owns the normalised adjacency of the bipartite graph as ONE CSR over the n_users + n_items nodes
// (users first: a user's row lists nu + item, an item's row lists users, i.e. the train matrix and its transpose, with the
// edge weight (deg_u deg_i)^-1/2 in both), the layer-0 tables in one buffer [E0_user | E0_item], Adam's two state buffers of
// the same layout and its step counter.
//
// E = P(E0), P = 1 / (L + 1) sum_{k = 0..L} A^k.  P is linear and symmetric, so dL/dE0 = P(G): the same hops serve both
// directions and nothing of the forward pass is kept but the running sum and two ping-pong buffers.
//
// An epoch's triplets lie on the device before the first step.  Then, with no host synchronisation in between:
//   order      once per epoch, all steps in one launch: each step's users and its items [positives | negatives] sorted by id,
//              stable, by counting (as ncf.hip orders its samples)
//   per step   hop x L     one lane group per node: H'_r = sum_{e in row r} w_e H[src_e], edges ascending, kLgcnAhead source
//                          rows in flight, the edge stream read a group's width at a time and one chunk ahead; S_r += H'_r,
//                          divided by L + 1 at the last layer.  A row longer than kLgcnPiece edges is cut into pieces, one
//                          group each, whose partial sums a second small launch adds in piece order.
//              loss        one wave per triplet: the two scores, softplus, sigmoid, the three squared norms
//              gradient    one thread per entry of G: bisects the step's sorted ids for its node and sums that node's
//                          gradient rows in sample order (float64, rounded once); zero elsewhere
//              hop x L     g = P(G)
//              adam        torch's dense update of every entry of both tables
//   losses     once per epoch: each step's terms summed by a fixed tree in float64
// No atomics; every sum has one fixed order, so the same inputs give the same bits.
#include "sparse_model.h"
#include "vae_device.h"

namespace chip {
namespace {

constexpr int kLgcnMaxD = 256, kLgcnMaxLayers = 8, kLgcnMaxStep = 16384;
constexpr int kLgcnPiece = 512;      // edges of one piece of a long row
constexpr int kLgcnAhead = 4;        // source rows in flight per lane group
constexpr int kLgcnBlock = 256;

// the adjacency as the kernels see it
struct LgcnGraph {
    int64_t n_nodes, n_pieces, n_split;
    const int64_t *ptr;          // [n_nodes + 1]
    const int32_t *idx;          // [2 nnz] source node of an edge
    const float *w;              // [2 nnz]
    const int32_t *piece_row;    // [n_pieces] the pieces of the split rows, a row's pieces adjacent and ascending
    const int64_t *piece_lo, *piece_hi;
    const int32_t *split_row;    // [n_split]
    const int64_t *split_first;  // [n_split + 1] a split row's pieces are [split_first[k], split_first[k + 1])
};

// where a hop's result goes: H' (unless this is the last layer), S = Sin + H' (divided by div at the last layer)
struct LgcnOut {
    float *hout;
    const float *sin;
    float *sout;
    int last;
    float div;
};

template <int VEC>
struct LgcnVec { float v[VEC]; };

template <int VEC>
__device__ inline LgcnVec<VEC> lgcn_load(const float *p) {
    LgcnVec<VEC> r;
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int VEC>
__device__ inline void lgcn_store(float *p, const LgcnVec<VEC> &r) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        *p = r.v[0];
    }
}

template <int VEC>
__device__ inline void lgcn_finish(const LgcnOut &o, int64_t at, const LgcnVec<VEC> &h) {
    if (!o.last) lgcn_store<VEC>(o.hout + at, h);
    LgcnVec<VEC> s = lgcn_load<VEC>(o.sin + at);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        s.v[q] = s.v[q] + h.v[q];
        if (o.last) s.v[q] = s.v[q] / o.div;
    }
    lgcn_store<VEC>(o.sout + at, s);
}

// ---- hop: one lane group of G lanes (a power of two, G * VEC * NC >= d) per task ---------------------------------------------------
// Tasks [0, n_nodes) are the nodes (a split row's task does nothing), tasks [n_nodes, n_nodes + n_pieces) the pieces of the
// split rows, whose sums go to part [n_pieces x d].  A lane holds the columns (lane + k G) VEC .. + VEC, k < NC.
template <int VEC, int NC>
__global__ __launch_bounds__(kLgcnBlock) void lgcn_hop_kernel(LgcnGraph g, int d, int G, const float *__restrict__ hin, float *part, LgcnOut o) {
    const int lane = (int)threadIdx.x & (G - 1);
    const int64_t task = (int64_t)blockIdx.x * (kLgcnBlock / G) + (int)threadIdx.x / G;
    if (task >= g.n_nodes + g.n_pieces) return;
    int64_t row, lo, hi;
    float *piece = nullptr;
    if (task < g.n_nodes) {
        row = task;
        lo = g.ptr[row];
        hi = g.ptr[row + 1];
        if (hi - lo > kLgcnPiece) return;
    } else {
        const int64_t p = task - g.n_nodes;
        row = g.piece_row[p];
        lo = g.piece_lo[p];
        hi = g.piece_hi[p];
        piece = part + p * d;
    }
    LgcnVec<VEC> acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[k].v[q] = 0.f;
    int32_t next_i = 0;
    float next_w = 0.f;
    if (lo + lane < hi) { next_i = g.idx[lo + lane]; next_w = g.w[lo + lane]; }
    for (int64_t e = lo; e < hi; e += G) {
        const int32_t cur_i = next_i;
        const float cur_w = next_w;
        const int cnt = (int)(hi - e < G ? hi - e : G);
        if (e + G + lane < hi) { next_i = g.idx[e + G + lane]; next_w = g.w[e + G + lane]; }   // the next chunk, ahead of use
        int j = 0;
        for (; j + kLgcnAhead <= cnt; j += kLgcnAhead) {
            LgcnVec<VEC> v[kLgcnAhead][NC];
            float w[kLgcnAhead];
#pragma unroll
            for (int a = 0; a < kLgcnAhead; ++a) {
                const int64_t src = (int64_t)__shfl(cur_i, j + a, G) * d;
                w[a] = __shfl(cur_w, j + a, G);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int c = (lane + k * G) * VEC;
                    if (c < d) v[a][k] = lgcn_load<VEC>(hin + src + c);
                }
            }
#pragma unroll
            for (int a = 0; a < kLgcnAhead; ++a)
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int c = (lane + k * G) * VEC;
                    if (c < d) {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) acc[k].v[q] = acc[k].v[q] + w[a] * v[a][k].v[q];
                    }
                }
        }
        for (; j < cnt; ++j) {
            const int64_t src = (int64_t)__shfl(cur_i, j, G) * d;
            const float w = __shfl(cur_w, j, G);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = (lane + k * G) * VEC;
                if (c < d) {
                    const LgcnVec<VEC> v = lgcn_load<VEC>(hin + src + c);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[k].v[q] = acc[k].v[q] + w * v.v[q];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int c = (lane + k * G) * VEC;
        if (c >= d) continue;
        if (piece) lgcn_store<VEC>(piece + c, acc[k]);
        else lgcn_finish<VEC>(o, row * d + c, acc[k]);
    }
}

// the split rows: H'_r = (piece 0 + piece 1) + piece 2 + ..., one lane group per row
template <int VEC, int NC>
__global__ __launch_bounds__(kLgcnBlock) void lgcn_combine_kernel(LgcnGraph g, int d, int G, const float *__restrict__ part, LgcnOut o) {
    const int lane = (int)threadIdx.x & (G - 1);
    const int64_t k0 = (int64_t)blockIdx.x * (kLgcnBlock / G) + (int)threadIdx.x / G;
    if (k0 >= g.n_split) return;
    const int64_t row = g.split_row[k0], first = g.split_first[k0], end = g.split_first[k0 + 1];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int c = (lane + k * G) * VEC;
        if (c >= d) continue;
        LgcnVec<VEC> acc = lgcn_load<VEC>(part + first * d + c);
        for (int64_t p = first + 1; p < end; ++p) {
            const LgcnVec<VEC> v = lgcn_load<VEC>(part + p * d + c);
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc.v[q] = acc.v[q] + v.v[q];
        }
        lgcn_finish<VEC>(o, row * d + c, acc);
    }
}

// ---- order: a step's ids sorted, stable (ncf.hip's counting order) ----------------------------------------------------------------
// grid (steps, ceil(2 max step / 256), 2): z = 0 sorts the step's users [n], z = 1 its items [2 n] = [positives | negatives],
// which lie at items[2 base ..].  order[.. + place] = the id's index in its list, sorted[.. + place] = the id.
__global__ __launch_bounds__(kLgcnBlock) void lgcn_order_kernel(const int64_t *__restrict__ step_ptr, const int32_t *__restrict__ users,
                                                                const int32_t *__restrict__ items, int32_t *order_u, int32_t *sorted_u,
                                                                int32_t *order_i, int32_t *sorted_i) {
    __shared__ int32_t sh[kLgcnBlock];
    const int64_t sbase = step_ptr[blockIdx.x];
    const int sn = (int)(step_ptr[blockIdx.x + 1] - sbase);
    const int64_t base = blockIdx.z ? 2 * sbase : sbase;
    const int n = blockIdx.z ? 2 * sn : sn;
    if ((int)blockIdx.y * kLgcnBlock >= n) return;
    const int32_t *ids = (blockIdx.z ? items : users) + base;
    const int s = (int)blockIdx.y * kLgcnBlock + (int)threadIdx.x;
    const int32_t mine = s < n ? ids[s] : 0;
    int place = 0;
    for (int t0 = 0; t0 < n; t0 += kLgcnBlock) {
        sh[threadIdx.x] = t0 + (int)threadIdx.x < n ? ids[t0 + threadIdx.x] : 0;
        __syncthreads();
        const int m = n - t0 < kLgcnBlock ? n - t0 : kLgcnBlock;
        for (int t = 0; t < m; ++t) {
            const int32_t other = sh[t];
            place += (other < mine || (other == mine && t0 + t < s)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (s < n) {
        (blockIdx.z ? order_i : order_u)[base + place] = s;
        (blockIdx.z ? sorted_i : sorted_u)[base + place] = mine;
    }
}

// ---- loss: one wave per triplet ----------------------------------------------------------------------------------------------------
__device__ inline float lgcn_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// E: the final embeddings [users | items]; pn: the step's [positives | negatives]; sig [n], bpr_t / reg_t [n] (the epoch's, at
// the step's base)
__global__ __launch_bounds__(kLgcnBlock) void lgcn_loss_kernel(const float *__restrict__ E, int d, int64_t n_users, int n,
                                                               const int32_t *__restrict__ users, const int32_t *__restrict__ pn, float *sig,
                                                               float *bpr_t, float *reg_t) {
    const int lane = (int)threadIdx.x & 63;
    const int b = (int)blockIdx.x * (kLgcnBlock / 64) + (int)threadIdx.x / 64;
    if (b >= n) return;
    const float *a = E + (int64_t)users[b] * d, *p = E + (n_users + pn[b]) * d, *q = E + (n_users + pn[n + b]) * d;
    float ap = 0.f, aq = 0.f, aa = 0.f, pp = 0.f, qq = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float x = a[c], y = p[c], z = q[c];
        ap = ap + x * y; aq = aq + x * z;
        aa = aa + x * x; pp = pp + y * y; qq = qq + z * z;
    }
    ap = lgcn_wave_sum(ap); aq = lgcn_wave_sum(aq);
    aa = lgcn_wave_sum(aa); pp = lgcn_wave_sum(pp); qq = lgcn_wave_sum(qq);
    if (lane == 0) {
        const float x = aq - ap;
        sig[b] = 1.f / (1.f + expf(-x));
        bpr_t[b] = x > 20.f ? x : log1pf(expf(x));   // F.softplus
        reg_t[b] = (aa + pp) + qq;
    }
}

// ---- gradient at the final embeddings: one thread per entry of G [users | items] ------------------------------------------------------
__device__ inline int lgcn_first(const int32_t *__restrict__ sorted, int n, int32_t id) {
    int lo = 0, hi = n;
    while (lo < hi) {   // the first place whose id is not below `id`
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kLgcnBlock) void lgcn_grad_kernel(const float *__restrict__ E, int d, int64_t n_users, int64_t total, int n,
                                                               const int32_t *__restrict__ users, const int32_t *__restrict__ pn,
                                                               const int32_t *__restrict__ order_u, const int32_t *__restrict__ sorted_u,
                                                               const int32_t *__restrict__ order_i, const int32_t *__restrict__ sorted_i,
                                                               const float *__restrict__ sig, float lambda, float *G) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t row = e / d;
    const int c = (int)(e % d);
    const float fn = (float)n;
    const float mine = E[e];
    double g = 0.0;
    if (row < n_users) {
        for (int at = lgcn_first(sorted_u, n, (int32_t)row); at < n && sorted_u[at] == (int32_t)row; ++at) {
            const int b = order_u[at];
            const float p = E[(n_users + pn[b]) * d + c], q = E[(n_users + pn[n + b]) * d + c];
            g += (double)((sig[b] * (q - p) + lambda * mine) / fn);
        }
    } else {
        const int32_t item = (int32_t)(row - n_users);
        for (int at = lgcn_first(sorted_i, 2 * n, item); at < 2 * n && sorted_i[at] == item; ++at) {
            const int s = order_i[at];
            const int b = s < n ? s : s - n;
            const float a = E[(int64_t)users[b] * d + c];
            const float sa = s < n ? -(sig[b] * a) : sig[b] * a;
            g += (double)((sa + lambda * mine) / fn);
        }
    }
    G[e] = (float)g;
}

__global__ __launch_bounds__(kLgcnBlock) void lgcn_adam_kernel(float *w, float *m, float *v, const float *__restrict__ g, int64_t total, VaeAdam a) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) vae_adam(w, m, v, e, g[e], a);
}

// ---- losses: one workgroup per step, a fixed tree in float64 ------------------------------------------------------------------------
__global__ __launch_bounds__(kLgcnBlock) void lgcn_step_loss_kernel(const int64_t *__restrict__ step_ptr, const float *__restrict__ bpr_t,
                                                                    const float *__restrict__ reg_t, double lambda, double *out) {
    __shared__ double sb[kLgcnBlock], sr[kLgcnBlock];
    const int64_t lo = step_ptr[blockIdx.x], hi = step_ptr[blockIdx.x + 1];
    double b = 0.0, r = 0.0;
    for (int64_t s = lo + threadIdx.x; s < hi; s += kLgcnBlock) { b += (double)bpr_t[s]; r += (double)reg_t[s]; }
    sb[threadIdx.x] = b;
    sr[threadIdx.x] = r;
    __syncthreads();
    for (int s = kLgcnBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sb[threadIdx.x] += sb[threadIdx.x + s]; sr[threadIdx.x] += sr[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)(hi - lo), bpr = sb[0] / n, reg = 0.5 * sr[0] / n;
        out[3 * (int64_t)blockIdx.x] = bpr + lambda * reg;
        out[3 * (int64_t)blockIdx.x + 1] = bpr;
        out[3 * (int64_t)blockIdx.x + 2] = reg;
    }
}

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_lightgcn : ModelHandle {
    int64_t n_users = 0, n_items = 0, nnz = 0, n_nodes = 0, total = 0;   // total: entries of a table pair
    int d = 0, L = 0, G = 1, vec = 1, nc = 1;
    int64_t t = 0;   // Adam's step counter
    int64_t n_pieces = 0, n_split = 0;
    DevBuf<int64_t> ptr, piece_lo, piece_hi, split_first;
    DevBuf<int32_t> idx, piece_row, split_row;
    DevBuf<float> ew;
    DevBuf<float> w, m, v;          // [E0_user | E0_item] and Adam's state
    DevBuf<float> E, Gr, gs, ha, hb, part;   // final embeddings, gradient at them, P(gradient), the hops' ping-pong, the pieces' sums
    // an epoch's triplets
    int64_t cap_samples = 0, cap_steps = 0;
    DevBuf<int32_t> users, pn, order_u, sorted_u, order_i, sorted_i;
    DevBuf<float> bpr_t, reg_t;
    DevBuf<int64_t> step_ptr;
    DevBuf<double> step_loss;
    int64_t cap_step = 0;
    DevBuf<float> sig;
};

static LgcnGraph lgcn_graph(cornac_hip_lightgcn_t h) {
    return LgcnGraph{h->n_nodes, h->n_pieces, h->n_split, h->ptr.p, h->idx.p, h->ew.p, h->piece_row.p, h->piece_lo.p, h->piece_hi.p,
                     h->split_row.p, h->split_first.p};
}

static unsigned lgcn_grid(int64_t n, int64_t per = kLgcnBlock) { return (unsigned)((n + per - 1) / per); }

template <int VEC, int NC>
static void lgcn_hop_as(cornac_hip_lightgcn_t h, const float *hin, const LgcnOut &o) {
    const LgcnGraph g = lgcn_graph(h);
    const int64_t per = kLgcnBlock / h->G;
    lgcn_hop_kernel<VEC, NC><<<lgcn_grid(g.n_nodes + g.n_pieces, per), kLgcnBlock, 0, h->stream>>>(g, h->d, h->G, hin, h->part.p, o);
    if (g.n_split) lgcn_combine_kernel<VEC, NC><<<lgcn_grid(g.n_split, per), kLgcnBlock, 0, h->stream>>>(g, h->d, h->G, h->part.p, o);
    HIP_CHECK(hipGetLastError());
}

static void lgcn_hop(cornac_hip_lightgcn_t h, const float *hin, const LgcnOut &o) {
    if (h->vec == 4) lgcn_hop_as<4, 1>(h, hin, o);
    else if (h->nc == 1) lgcn_hop_as<1, 1>(h, hin, o);
    else lgcn_hop_as<1, 4>(h, hin, o);
}

// out = P(in): L hops; in and out are distinct table pairs
static void lgcn_propagate(cornac_hip_lightgcn_t h, const float *in, float *out) {
    if (h->L == 0) {
        HIP_CHECK(hipMemcpyAsync(out, in, (size_t)h->total * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        return;
    }
    const float *cur = in;
    for (int k = 1; k <= h->L; ++k) {
        float *dst = (k & 1) ? h->ha.p : h->hb.p;
        lgcn_hop(h, cur, LgcnOut{dst, k == 1 ? in : out, out, k == h->L ? 1 : 0, (float)(h->L + 1)});
        cur = dst;
    }
}

int cornac_hip_lightgcn_create(cornac_hip_lightgcn_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                               const int32_t *indices, int emb_size, int num_layers) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "lightgcn: sizes must be positive");
        REQUIRE(n_users + n_items < (1ll << 31), "lightgcn: n_users + n_items must be below 2^31");
        REQUIRE(emb_size >= 1 && emb_size <= kLgcnMaxD, "lightgcn: emb_size = %d is outside the supported range 1 <= emb_size <= %d",
                emb_size, kLgcnMaxD);
        REQUIRE(num_layers >= 0 && num_layers <= kLgcnMaxLayers, "lightgcn: num_layers = %d is outside the supported range 0 <= num_layers <= %d",
                num_layers, kLgcnMaxLayers);
        check_csr("lightgcn", "the training matrix", n_users, n_items, indptr, indices, nullptr, kCsrNoValues);
        const int64_t nnz = indptr[n_users];
        REQUIRE(nnz < (1ll << 31), "lightgcn: %lld stored entries are more than the supported 2^31 - 1", (long long)nnz);
        std::unique_ptr<cornac_hip_lightgcn> h(new cornac_hip_lightgcn());
        h->n_users = n_users; h->n_items = n_items; h->nnz = nnz;
        h->n_nodes = n_users + n_items;
        h->d = emb_size; h->L = num_layers;
        h->total = h->n_nodes * emb_size;
        h->vec = emb_size % 4 == 0 ? 4 : 1;
        const int lanes = (emb_size + h->vec - 1) / h->vec;
        h->G = 1;
        while (h->G < lanes && h->G < 64) h->G *= 2;
        h->nc = (lanes + h->G - 1) / h->G > 1 ? 4 : 1;
        // the adjacency over all nodes and its weights (lightgcn.py:31-39: pow(float(deg_src) * float(deg_dst), -0.5) in float32)
        const HostCsr T = transpose_csr(n_users, n_items, indptr, indices, nullptr);
        const int64_t N = h->n_nodes;
        std::vector<int64_t> ptr((size_t)N + 1);
        std::vector<int32_t> idx((size_t)(2 * nnz));
        std::vector<float> ew((size_t)(2 * nnz));
        auto weight = [&](int64_t du, int64_t di) { return (float)std::pow((double)((float)du * (float)di), -0.5); };
        for (int64_t u = 0; u <= n_users; ++u) ptr[(size_t)u] = indptr[u];
        for (int64_t i = 1; i <= n_items; ++i) ptr[(size_t)(n_users + i)] = nnz + T.ptr[(size_t)i];
        for (int64_t u = 0; u < n_users; ++u)
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) {
                const int64_t i = indices[e];
                idx[(size_t)e] = (int32_t)(n_users + i);
                ew[(size_t)e] = weight(indptr[u + 1] - indptr[u], T.ptr[(size_t)i + 1] - T.ptr[(size_t)i]);
            }
        for (int64_t i = 0; i < n_items; ++i)
            for (int64_t e = T.ptr[(size_t)i]; e < T.ptr[(size_t)i + 1]; ++e) {
                const int64_t u = T.idx[(size_t)e];
                idx[(size_t)(nnz + e)] = (int32_t)u;
                ew[(size_t)(nnz + e)] = weight(indptr[u + 1] - indptr[u], T.ptr[(size_t)i + 1] - T.ptr[(size_t)i]);
            }
        // the long rows' pieces
        std::vector<int32_t> piece_row, split_row;
        std::vector<int64_t> piece_lo, piece_hi, split_first;
        for (int64_t r = 0; r < N; ++r) {
            const int64_t lo = ptr[(size_t)r], hi = ptr[(size_t)r + 1];
            if (hi - lo <= kLgcnPiece) continue;
            split_row.push_back((int32_t)r);
            split_first.push_back((int64_t)piece_row.size());
            for (int64_t a = lo; a < hi; a += kLgcnPiece) {
                piece_row.push_back((int32_t)r);
                piece_lo.push_back(a);
                piece_hi.push_back(std::min(a + kLgcnPiece, hi));
            }
        }
        split_first.push_back((int64_t)piece_row.size());
        h->n_pieces = (int64_t)piece_row.size();
        h->n_split = (int64_t)split_row.size();
        h->open(device);
        const char *nm = "lightgcn", *graph = "the graph's pointers, indices and weights";
        alloc_named(h->ptr, (size_t)N + 1, nm, graph);
        alloc_named(h->idx, (size_t)(2 * nnz), nm, graph);
        alloc_named(h->ew, (size_t)(2 * nnz), nm, graph);
        h->ptr.upload(ptr.data(), (size_t)N + 1, h->stream);
        if (nnz) {
            h->idx.upload(idx.data(), (size_t)(2 * nnz), h->stream);
            h->ew.upload(ew.data(), (size_t)(2 * nnz), h->stream);
        }
        if (h->n_split) {
            const char *pieces = "the long rows' pieces";
            alloc_named(h->piece_row, (size_t)h->n_pieces, nm, pieces);
            alloc_named(h->piece_lo, (size_t)h->n_pieces, nm, pieces);
            alloc_named(h->piece_hi, (size_t)h->n_pieces, nm, pieces);
            alloc_named(h->split_row, (size_t)h->n_split, nm, pieces);
            alloc_named(h->split_first, (size_t)h->n_split + 1, nm, pieces);
            alloc_named(h->part, (size_t)(h->n_pieces * emb_size), nm, pieces);
            h->piece_row.upload(piece_row.data(), (size_t)h->n_pieces, h->stream);
            h->piece_lo.upload(piece_lo.data(), (size_t)h->n_pieces, h->stream);
            h->piece_hi.upload(piece_hi.data(), (size_t)h->n_pieces, h->stream);
            h->split_row.upload(split_row.data(), (size_t)h->n_split, h->stream);
            h->split_first.upload(split_first.data(), (size_t)h->n_split + 1, h->stream);
        }
        for (DevBuf<float> *b : {&h->w, &h->m, &h->v, &h->E, &h->Gr, &h->gs, &h->ha, &h->hb}) {
            alloc_named(*b, (size_t)h->total, nm, "the tables, Adam's state and the propagation buffers");
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_lightgcn_destroy(cornac_hip_lightgcn_t h) { return destroy_handle(h); }

static void lgcn_put(cornac_hip_lightgcn_t h, DevBuf<float> &buf, const float *user, const float *item) {
    const size_t nu = (size_t)(h->n_users * h->d), ni = (size_t)(h->n_items * h->d);
    if (user) HIP_CHECK(hipMemcpyAsync(buf.p, user, nu * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (item) HIP_CHECK(hipMemcpyAsync(buf.p + nu, item, ni * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

static void lgcn_get(cornac_hip_lightgcn_t h, const DevBuf<float> &buf, float *user, float *item) {
    const size_t nu = (size_t)(h->n_users * h->d), ni = (size_t)(h->n_items * h->d);
    if (user) HIP_CHECK(hipMemcpyAsync(user, buf.p, nu * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (item) HIP_CHECK(hipMemcpyAsync(item, buf.p + nu, ni * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

int cornac_hip_lightgcn_set_params(cornac_hip_lightgcn_t h, const float *user, const float *item) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_put(h, h->w, user, item);
    });
}

int cornac_hip_lightgcn_get_params(cornac_hip_lightgcn_t h, float *user, float *item) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_get(h, h->w, user, item);
    });
}

int cornac_hip_lightgcn_get_state(cornac_hip_lightgcn_t h, float *m_user, float *m_item, float *v_user, float *v_item, int64_t *t) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_get(h, h->m, m_user, m_item);
        lgcn_get(h, h->v, v_user, v_item);
        if (t) *t = h->t;
    });
}

int cornac_hip_lightgcn_reset_optimizer(cornac_hip_lightgcn_t h) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        HIP_CHECK(hipMemsetAsync(h->m.p, 0, h->m.n * sizeof(float), h->stream));
        HIP_CHECK(hipMemsetAsync(h->v.p, 0, h->v.n * sizeof(float), h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->t = 0;
    });
}

int cornac_hip_lightgcn_propagate(cornac_hip_lightgcn_t h, float *user_out, float *item_out) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_propagate(h, h->w.p, h->E.p);
        lgcn_get(h, h->E, user_out, item_out);
    });
}

static void lgcn_ensure_epoch(cornac_hip_lightgcn_t h, int64_t samples, int64_t steps, int64_t max_n) {
    const char *nm = "lightgcn", *what = "an epoch's triplets";
    if (samples > h->cap_samples) {
        for (DevBuf<int32_t> *b : {&h->users, &h->order_u, &h->sorted_u}) alloc_named(*b, (size_t)samples, nm, what);
        for (DevBuf<int32_t> *b : {&h->pn, &h->order_i, &h->sorted_i}) alloc_named(*b, (size_t)(2 * samples), nm, what);
        alloc_named(h->bpr_t, (size_t)samples, nm, what);
        alloc_named(h->reg_t, (size_t)samples, nm, what);
        h->cap_samples = samples;
    }
    if (steps > h->cap_steps) {
        alloc_named(h->step_ptr, (size_t)steps + 1, nm, what);
        alloc_named(h->step_loss, (size_t)(3 * steps), nm, what);
        h->cap_steps = steps;
    }
    if (max_n > h->cap_step) {
        alloc_named(h->sig, (size_t)max_n, nm, "a step's sigmoids");
        h->cap_step = max_n;
    }
}

int cornac_hip_lightgcn_fit_epoch(cornac_hip_lightgcn_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users,
                                  const int32_t *pos, const int32_t *neg, float lr, float lambda_reg, double *loss_out,
                                  double *bpr_out, double *reg_out) {
    return guarded([&] {
        // (the steps' shape is checked before the handle: it needs no device)
        REQUIRE(steps >= 1 && steps < (1ll << 31), "lightgcn: the number of steps must be in 1 .. 2^31 - 1");
        REQUIRE(step_ptr != nullptr, "lightgcn: step_ptr is NULL");
        REQUIRE(step_ptr[0] == 0, "lightgcn: step_ptr does not start at 0");
        int64_t max_n = 0;
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t n = step_ptr[s + 1] - step_ptr[s];
            REQUIRE(n >= 1 && n <= kLgcnMaxStep, "lightgcn: step %lld has %lld triplets, outside the supported range 1 <= batch_size <= %d",
                    (long long)s, (long long)n, kLgcnMaxStep);
            max_n = std::max(max_n, n);
        }
        check_handle(h, "lightgcn handle");
        REQUIRE(users && pos && neg, "lightgcn: users / pos / neg are NULL");
        REQUIRE(std::isfinite(lr) && std::isfinite(lambda_reg), "lightgcn: lr and lambda_reg must be finite");
        const int64_t total = step_ptr[steps];
        std::vector<int32_t> pn((size_t)(2 * total));
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t base = step_ptr[s], n = step_ptr[s + 1] - base;
            for (int64_t b = 0; b < n; ++b) {
                const int64_t q = base + b;
                REQUIRE(users[q] >= 0 && users[q] < h->n_users, "lightgcn: user %d out of range", users[q]);
                REQUIRE(pos[q] >= 0 && pos[q] < h->n_items, "lightgcn: positive item %d out of range", pos[q]);
                REQUIRE(neg[q] >= 0 && neg[q] < h->n_items, "lightgcn: negative item %d out of range", neg[q]);
                pn[(size_t)(2 * base + b)] = pos[q];
                pn[(size_t)(2 * base + n + b)] = neg[q];
            }
        }
        lgcn_ensure_epoch(h, total, steps, max_n);
        h->users.upload(users, (size_t)total, h->stream);
        h->pn.upload(pn.data(), (size_t)(2 * total), h->stream);
        h->step_ptr.upload(step_ptr, (size_t)steps + 1, h->stream);
        lgcn_order_kernel<<<dim3((unsigned)steps, lgcn_grid(2 * max_n), 2), kLgcnBlock, 0, h->stream>>>(
            h->step_ptr.p, h->users.p, h->pn.p, h->order_u.p, h->sorted_u.p, h->order_i.p, h->sorted_i.p);
        HIP_CHECK(hipGetLastError());
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t base = step_ptr[s], n = step_ptr[s + 1] - base;
            h->t += 1;
            const double bc1 = 1.0 - std::pow(0.9, (double)h->t), bc2 = 1.0 - std::pow(0.999, (double)h->t);
            const VaeAdam adam{(float)(1.0 - 0.9), 0.999f, (float)(1.0 - 0.999), (float)((double)lr / bc1), (float)std::sqrt(bc2), 1e-8f};
            lgcn_propagate(h, h->w.p, h->E.p);
            lgcn_loss_kernel<<<lgcn_grid(n, kLgcnBlock / 64), kLgcnBlock, 0, h->stream>>>(
                h->E.p, h->d, h->n_users, (int)n, h->users.p + base, h->pn.p + 2 * base, h->sig.p, h->bpr_t.p + base, h->reg_t.p + base);
            lgcn_grad_kernel<<<lgcn_grid(h->total), kLgcnBlock, 0, h->stream>>>(
                h->E.p, h->d, h->n_users, h->total, (int)n, h->users.p + base, h->pn.p + 2 * base, h->order_u.p + base, h->sorted_u.p + base,
                h->order_i.p + 2 * base, h->sorted_i.p + 2 * base, h->sig.p, lambda_reg, h->Gr.p);
            HIP_CHECK(hipGetLastError());
            lgcn_propagate(h, h->Gr.p, h->gs.p);
            lgcn_adam_kernel<<<lgcn_grid(h->total), kLgcnBlock, 0, h->stream>>>(h->w.p, h->m.p, h->v.p, h->gs.p, h->total, adam);
            HIP_CHECK(hipGetLastError());
        }
        lgcn_step_loss_kernel<<<(unsigned)steps, kLgcnBlock, 0, h->stream>>>(h->step_ptr.p, h->bpr_t.p, h->reg_t.p, (double)lambda_reg,
                                                                            h->step_loss.p);
        HIP_CHECK(hipGetLastError());
        std::vector<double> losses((size_t)(3 * steps));
        h->step_loss.download(losses.data(), (size_t)(3 * steps), h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));   // (pn is the upload's source)
        for (int64_t s = 0; s < steps; ++s) {
            if (loss_out) loss_out[s] = losses[(size_t)(3 * s)];
            if (bpr_out) bpr_out[s] = losses[(size_t)(3 * s + 1)];
            if (reg_out) reg_out[s] = losses[(size_t)(3 * s + 2)];
        }
    });
}

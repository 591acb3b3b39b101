// The user-item graph of the two graph models (lightgcn.hip, ngcf.hip): the normalised adjacency as ONE CSR over the
// n_users + n_items nodes with its host builder, the hop over it, the order of a step's ids, the BPR loss and gradient rows
// at the final embeddings, Adam's dense pass and the steps' losses.  Moved here from lightgcn.hip as they stood (as rng.h took
// the Feistel code): their arithmetic is LightGCN's, and its tests hold it in place.  What a hop does with a finished row
// segment is the template parameter EPI:
//     template <int VEC> __device__ void finish(int64_t row, int c, int d, const LgcnVec<VEC> &h) const
// gets the columns c .. c + VEC of row `row` of A H (d: the width of the hop).
// The kernels sit in an unnamed namespace: every source that includes this header gets its own copies.
#pragma once
#include "vae_host.h"

namespace chip {
namespace {

constexpr int kLgcnMaxD = 256, kLgcnMaxLayers = 8, kLgcnMaxStep = 16384;
constexpr int kLgcnPiece = 512;      // edges of one piece of a long row
constexpr int kLgcnAhead = 4;        // source rows in flight per lane group
constexpr int kLgcnBlock = 256;
static_assert(kLgcnBlock == kVaeBlock, "grid() counts workgroups of kVaeBlock by default");

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

// ---- hop: one lane group of G lanes (a power of two, G * VEC * NC >= d) per task ---------------------------------------------------
// Tasks [0, n_nodes) are the nodes (a split row's task does nothing), tasks [n_nodes, n_nodes + n_pieces) the pieces of the
// split rows, whose sums go to part [n_pieces x d].  A lane holds the columns (lane + k G) VEC .. + VEC, k < NC.
template <int VEC, int NC, class EPI>
__global__ __launch_bounds__(kLgcnBlock) void lgcn_hop_kernel(LgcnGraph g, int d, int G, const float *__restrict__ hin, float *part, EPI o) {
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
        else o.template finish<VEC>(row, c, d, acc[k]);
    }
}

// the split rows: H'_r = (piece 0 + piece 1) + piece 2 + ..., one lane group per row
template <int VEC, int NC, class EPI>
__global__ __launch_bounds__(kLgcnBlock) void lgcn_combine_kernel(LgcnGraph g, int d, int G, const float *__restrict__ part, EPI o) {
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
        o.template finish<VEC>(row, c, d, acc);
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

// ---- host: the graph on the device ----------------------------------------------------------------------------------------------------
// the lane group, the vector width and the column count of a hop of width d
struct LgcnShape {
    int G, vec, nc;
    explicit LgcnShape(int d) {
        vec = d % 4 == 0 ? 4 : 1;
        const int lanes = (d + vec - 1) / vec;
        G = 1;
        while (G < lanes && G < 64) G *= 2;
        nc = (lanes + G - 1) / G > 1 ? 4 : 1;
    }
};

struct LgcnGraphDev {
    int64_t n_users = 0, n_items = 0, nnz = 0, n_nodes = 0, n_pieces = 0, n_split = 0;
    DevBuf<int64_t> ptr, piece_lo, piece_hi, split_first;
    DevBuf<int32_t> idx, piece_row, split_row;
    DevBuf<float> ew, part;   // part: the pieces' sums [n_pieces x the widest hop]
    // the host's copy, from build() to upload()
    std::vector<int64_t> h_ptr, h_piece_lo, h_piece_hi, h_split_first;
    std::vector<int32_t> h_idx, h_piece_row, h_split_row;
    std::vector<float> h_ew;

    // the adjacency over all nodes and its weights (lightgcn.py:31-39, ngcf.py:110-117: pow(float(deg_src) * float(deg_dst), -0.5)
    // in float32) and the long rows' pieces.  Needs no device.
    void build(const char *nm, int64_t nu, int64_t ni, const int64_t *indptr, const int32_t *indices) {
        REQUIRE(nu > 0 && ni > 0, "%s: sizes must be positive", nm);
        REQUIRE(nu + ni < (1ll << 31), "%s: n_users + n_items must be below 2^31", nm);
        check_csr(nm, "the training matrix", nu, ni, indptr, indices, nullptr, kCsrNoValues);
        nnz = indptr[nu];
        REQUIRE(nnz < (1ll << 31), "%s: %lld stored entries are more than the supported 2^31 - 1", nm, (long long)nnz);
        n_users = nu; n_items = ni;
        n_nodes = nu + ni;
        const HostCsr T = transpose_csr(n_users, n_items, indptr, indices, nullptr);
        const int64_t N = n_nodes;
        h_ptr.resize((size_t)N + 1);
        h_idx.resize((size_t)(2 * nnz));
        h_ew.resize((size_t)(2 * nnz));
        auto weight = [&](int64_t du, int64_t di) { return (float)std::pow((double)((float)du * (float)di), -0.5); };
        for (int64_t u = 0; u <= n_users; ++u) h_ptr[(size_t)u] = indptr[u];
        for (int64_t i = 1; i <= n_items; ++i) h_ptr[(size_t)(n_users + i)] = nnz + T.ptr[(size_t)i];
        for (int64_t u = 0; u < n_users; ++u)
            for (int64_t e = indptr[u]; e < indptr[u + 1]; ++e) {
                const int64_t i = indices[e];
                h_idx[(size_t)e] = (int32_t)(n_users + i);
                h_ew[(size_t)e] = weight(indptr[u + 1] - indptr[u], T.ptr[(size_t)i + 1] - T.ptr[(size_t)i]);
            }
        for (int64_t i = 0; i < n_items; ++i)
            for (int64_t e = T.ptr[(size_t)i]; e < T.ptr[(size_t)i + 1]; ++e) {
                const int64_t u = T.idx[(size_t)e];
                h_idx[(size_t)(nnz + e)] = (int32_t)u;
                h_ew[(size_t)(nnz + e)] = weight(indptr[u + 1] - indptr[u], T.ptr[(size_t)i + 1] - T.ptr[(size_t)i]);
            }
        for (int64_t r = 0; r < N; ++r) {
            const int64_t lo = h_ptr[(size_t)r], hi = h_ptr[(size_t)r + 1];
            if (hi - lo <= kLgcnPiece) continue;
            h_split_row.push_back((int32_t)r);
            h_split_first.push_back((int64_t)h_piece_row.size());
            for (int64_t a = lo; a < hi; a += kLgcnPiece) {
                h_piece_row.push_back((int32_t)r);
                h_piece_lo.push_back(a);
                h_piece_hi.push_back(std::min(a + kLgcnPiece, hi));
            }
        }
        h_split_first.push_back((int64_t)h_piece_row.size());
        n_pieces = (int64_t)h_piece_row.size();
        n_split = (int64_t)h_split_row.size();
    }

    // the rows' weight sums c_r = sum_e w_e, edges ascending in float64, rounded once
    std::vector<float> row_sums() const {
        std::vector<float> c((size_t)n_nodes);
        for (int64_t r = 0; r < n_nodes; ++r) {
            double s = 0.0;
            for (int64_t e = h_ptr[(size_t)r]; e < h_ptr[(size_t)r + 1]; ++e) s += (double)h_ew[(size_t)e];
            c[(size_t)r] = (float)s;
        }
        return c;
    }

    // after the handle's open(): allocates and copies; width: the widest hop.  Synchronise `stream` before the host copy goes.
    void upload(const char *nm, int width, hipStream_t stream) {
        const char *graph = "the graph's pointers, indices and weights";
        const size_t N = (size_t)n_nodes;
        alloc_named(ptr, N + 1, nm, graph);
        alloc_named(idx, (size_t)(2 * nnz), nm, graph);
        alloc_named(ew, (size_t)(2 * nnz), nm, graph);
        ptr.upload(h_ptr.data(), N + 1, stream);
        if (nnz) {
            idx.upload(h_idx.data(), (size_t)(2 * nnz), stream);
            ew.upload(h_ew.data(), (size_t)(2 * nnz), stream);
        }
        if (n_split) {
            const char *pieces = "the long rows' pieces";
            alloc_named(piece_row, (size_t)n_pieces, nm, pieces);
            alloc_named(piece_lo, (size_t)n_pieces, nm, pieces);
            alloc_named(piece_hi, (size_t)n_pieces, nm, pieces);
            alloc_named(split_row, (size_t)n_split, nm, pieces);
            alloc_named(split_first, (size_t)n_split + 1, nm, pieces);
            alloc_named(part, (size_t)(n_pieces * width), nm, pieces);
            piece_row.upload(h_piece_row.data(), (size_t)n_pieces, stream);
            piece_lo.upload(h_piece_lo.data(), (size_t)n_pieces, stream);
            piece_hi.upload(h_piece_hi.data(), (size_t)n_pieces, stream);
            split_row.upload(h_split_row.data(), (size_t)n_split, stream);
            split_first.upload(h_split_first.data(), (size_t)n_split + 1, stream);
        }
    }

    void drop_host() {
        for (auto *v : {&h_ptr, &h_piece_lo, &h_piece_hi, &h_split_first}) std::vector<int64_t>().swap(*v);
        for (auto *v : {&h_idx, &h_piece_row, &h_split_row}) std::vector<int32_t>().swap(*v);
        std::vector<float>().swap(h_ew);
    }

    LgcnGraph view() const {
        return LgcnGraph{n_nodes, n_pieces, n_split, ptr.p, idx.p, ew.p, piece_row.p, piece_lo.p, piece_hi.p, split_row.p, split_first.p};
    }
};

template <int VEC, int NC, class EPI>
void lgcn_hop_as(const LgcnGraphDev &gd, int d, int G, const float *hin, const EPI &o, hipStream_t stream) {
    const LgcnGraph g = gd.view();
    const int64_t per = kLgcnBlock / G;
    lgcn_hop_kernel<VEC, NC, EPI><<<grid(g.n_nodes + g.n_pieces, per), kLgcnBlock, 0, stream>>>(g, d, G, hin, gd.part.p, o);
    if (g.n_split) lgcn_combine_kernel<VEC, NC, EPI><<<grid(g.n_split, per), kLgcnBlock, 0, stream>>>(g, d, G, gd.part.p, o);
    HIP_CHECK(hipGetLastError());
}

// one hop of width d: o.finish gets every row segment of A hin
template <class EPI>
void lgcn_hop(const LgcnGraphDev &gd, int d, const float *hin, const EPI &o, hipStream_t stream) {
    const LgcnShape s(d);
    if (s.vec == 4) lgcn_hop_as<4, 1>(gd, d, s.G, hin, o, stream);
    else if (s.nc == 1) lgcn_hop_as<1, 1>(gd, d, s.G, hin, o, stream);
    else lgcn_hop_as<1, 4>(gd, d, s.G, hin, o, stream);
}

// ---- host: an epoch's triplets on the device --------------------------------------------------------------------------------------
struct LgcnEpoch {
    int64_t cap_samples = 0, cap_steps = 0, cap_step = 0;
    DevBuf<int32_t> users, pn, order_u, sorted_u, order_i, sorted_i;
    DevBuf<float> bpr_t, reg_t, sig;
    DevBuf<int64_t> step_ptr;
    DevBuf<double> step_loss;
    std::vector<int32_t> h_pn;   // the upload's source: lives until the stream is synchronised

    // the steps' shape: needs no device.  Returns the longest step.
    static int64_t check_steps(const char *nm, int64_t steps, const int64_t *step_ptr) {
        REQUIRE(steps >= 1 && steps < (1ll << 31), "%s: the number of steps must be in 1 .. 2^31 - 1", nm);
        REQUIRE(step_ptr != nullptr, "%s: step_ptr is NULL", nm);
        REQUIRE(step_ptr[0] == 0, "%s: step_ptr does not start at 0", nm);
        int64_t max_n = 0;
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t n = step_ptr[s + 1] - step_ptr[s];
            REQUIRE(n >= 1 && n <= kLgcnMaxStep, "%s: step %lld has %lld triplets, outside the supported range 1 <= batch_size <= %d", nm,
                    (long long)s, (long long)n, kLgcnMaxStep);
            max_n = std::max(max_n, n);
        }
        return max_n;
    }

    // checks the ids, uploads the triplets and orders every step's ids
    void stage(const char *nm, int64_t n_users, int64_t n_items, int64_t steps, int64_t max_n, const int64_t *sp, const int32_t *u,
               const int32_t *pos, const int32_t *neg, hipStream_t stream) {
        REQUIRE(u && pos && neg, "%s: users / pos / neg are NULL", nm);
        const int64_t total = sp[steps];
        h_pn.resize((size_t)(2 * total));
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t base = sp[s], n = sp[s + 1] - base;
            for (int64_t b = 0; b < n; ++b) {
                const int64_t q = base + b;
                REQUIRE(u[q] >= 0 && u[q] < n_users, "%s: user %d out of range", nm, u[q]);
                REQUIRE(pos[q] >= 0 && pos[q] < n_items, "%s: positive item %d out of range", nm, pos[q]);
                REQUIRE(neg[q] >= 0 && neg[q] < n_items, "%s: negative item %d out of range", nm, neg[q]);
                h_pn[(size_t)(2 * base + b)] = pos[q];
                h_pn[(size_t)(2 * base + n + b)] = neg[q];
            }
        }
        const char *what = "an epoch's triplets";
        if (total > cap_samples) {
            for (DevBuf<int32_t> *b : {&users, &order_u, &sorted_u}) alloc_named(*b, (size_t)total, nm, what);
            for (DevBuf<int32_t> *b : {&pn, &order_i, &sorted_i}) alloc_named(*b, (size_t)(2 * total), nm, what);
            alloc_named(bpr_t, (size_t)total, nm, what);
            alloc_named(reg_t, (size_t)total, nm, what);
            cap_samples = total;
        }
        if (steps > cap_steps) {
            alloc_named(step_ptr, (size_t)steps + 1, nm, what);
            alloc_named(step_loss, (size_t)(3 * steps), nm, what);
            cap_steps = steps;
        }
        if (max_n > cap_step) {
            alloc_named(sig, (size_t)max_n, nm, "a step's sigmoids");
            cap_step = max_n;
        }
        users.upload(u, (size_t)total, stream);
        pn.upload(h_pn.data(), (size_t)(2 * total), stream);
        step_ptr.upload(sp, (size_t)steps + 1, stream);
        lgcn_order_kernel<<<dim3((unsigned)steps, grid(2 * max_n), 2), kLgcnBlock, 0, stream>>>(step_ptr.p, users.p, pn.p, order_u.p,
                                                                                                sorted_u.p, order_i.p, sorted_i.p);
        HIP_CHECK(hipGetLastError());
    }

    // a step's loss terms, then the gradient rows at the final embeddings E [n_nodes x d] into G
    void loss_and_gradient(const float *E, int d, int64_t n_users, int64_t n_nodes, int64_t base, int64_t n, float lambda, float *G,
                           hipStream_t stream) {
        lgcn_loss_kernel<<<grid(n, kLgcnBlock / 64), kLgcnBlock, 0, stream>>>(E, d, n_users, (int)n, users.p + base, pn.p + 2 * base, sig.p,
                                                                              bpr_t.p + base, reg_t.p + base);
        lgcn_grad_kernel<<<grid(n_nodes * d), kLgcnBlock, 0, stream>>>(E, d, n_users, n_nodes * d, (int)n, users.p + base, pn.p + 2 * base,
                                                                       order_u.p + base, sorted_u.p + base, order_i.p + 2 * base,
                                                                       sorted_i.p + 2 * base, sig.p, lambda, G);
        HIP_CHECK(hipGetLastError());
    }

    // every step's three losses to the host; synchronises the stream
    void losses(int64_t steps, double lambda, double *loss_out, double *bpr_out, double *reg_out, hipStream_t stream) {
        lgcn_step_loss_kernel<<<(unsigned)steps, kLgcnBlock, 0, stream>>>(step_ptr.p, bpr_t.p, reg_t.p, lambda, step_loss.p);
        HIP_CHECK(hipGetLastError());
        std::vector<double> out((size_t)(3 * steps));
        step_loss.download(out.data(), (size_t)(3 * steps), stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        for (int64_t s = 0; s < steps; ++s) {
            if (loss_out) loss_out[s] = out[(size_t)(3 * s)];
            if (bpr_out) bpr_out[s] = out[(size_t)(3 * s + 1)];
            if (reg_out) reg_out[s] = out[(size_t)(3 * s + 2)];
        }
    }
};

}  // namespace
}  // namespace chip

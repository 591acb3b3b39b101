// Neighbourhood models (UserKNN / ItemKNN) on gfx950: the similarity table and the top-k neighbour scoring of
// cornac/models/knn/similarity.pyx (+ similarity.h), all in float64.
//
// Similarity (compute_similarity, similarity.pyx:51-105).  One workgroup owns one row r of W and three dense accumulators of
// n_rows doubles in device scratch (S, d1, d2).  It walks r's entries (c, w) in stored order; the threads share column c's
// entries (one target each: a column holds a row at most once) and a workgroup barrier separates two columns, so every
// S[r,i] is summed in the reference's order, each *, + rounded on its own (the tree is built with -ffp-contract=off).  No
// float atomics anywhere.  The quotient is S / sqrt(d1 * d2): what the reference's extension computes as compiled
// (-ffast-math folds sqrt(d1) * sqrt(d2)).  Rows run in passes of rows_per_pass; after a pass its non-zero quotients are
// counted, prefixed and compacted to CSR on the device into a chunk sized exactly for them.
//
// Scoring (compute_score / compute_score_single, similarity.pyx:108-201; TopK and SparseNeighbors of similarity.h).  One wave
// per (user, item).  The candidates of N's row i -- entries (nn, s) with v[nn] != 0, v the user's dense row of Q -- are
// compacted in the reference's feed order (reverse stored order) into a per-workgroup buffer.  With more than k of them the
// k-th largest weight T is found by an 8-round radix select over order-preserving 64-bit keys, and the survivors of the
// reference's heap are stated without replaying it: every candidate above T; of the first k candidates (feed order) with
// weight >= T, those at T, minus as many of their smallest ratings as there are candidates above T behind them.
// The survivors are summed in one fixed order (lane-strided partial sums, then a butterfly).
#include "sparse_model.h"


namespace chip {
namespace {

constexpr int kKnnBlock = 256;
constexpr int kKnnWave = 64;
constexpr int kKnnMaxK = CORNAC_HIP_KNN_MAX_K;
static_assert(kKnnMaxK <= kKnnWave, "the tie stage keeps one weight-T member of P per lane");

constexpr int64_t kKnnDenseBytes = 64ll << 20;   // a scoring chunk's dense rows of Q

// ---- similarity ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKnnBlock) void knn_sim_rows_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, const double *__restrict__ row_val,
    const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ col_idx, const double *__restrict__ col_val, int64_t n_rows,
    int64_t r0, double *S_all, double *D1_all, double *D2_all, int *counts) {
    const int64_t b = blockIdx.x, r = r0 + b;
    double *S = S_all + b * n_rows, *D1 = D1_all + b * n_rows, *D2 = D2_all + b * n_rows;
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    for (int64_t i = threadIdx.x; i < n_rows; i += kKnnBlock) {
        S[i] = 0.0;
        D1[i] = 0.0;
        D2[i] = 0.0;
    }
    __syncthreads();
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {   // (uniform: every thread walks the row's entries)
        const int32_t c = row_idx[e];
        const double w = row_val[e];
        for (int64_t j = col_ptr[c] + threadIdx.x; j < col_ptr[c + 1]; j += kKnnBlock) {
            const int32_t i = col_idx[j];
            const double x = col_val[j];
            S[i] += x * w;
            if (w != 0.0 && x != 0.0) {
                D1[i] += w * w;
                D2[i] += x * x;
            }
        }
        __syncthreads();   // the next column may hit the same targets: its additions come after these
    }
    int mine = 0;
    for (int64_t i = threadIdx.x; i < n_rows; i += kKnnBlock) {
        const double s = S[i];
        double q = 0.0;
        if (s != 0.0) q = s / sqrt(D1[i] * D2[i]);
        S[i] = q;
        mine += q != 0.0;
    }
    if (mine) atomicAdd(&cnt, mine);   // (an integer count: its order does not matter)
    __syncthreads();
    if (threadIdx.x == 0) counts[b] = cnt;
}

// offs[j] = counts[0] + .. + counts[j-1] (offs[R] = the pass's total), indptr_out[j + 1] = base + offs[j + 1]; one workgroup
__global__ __launch_bounds__(kKnnBlock) void knn_prefix_kernel(const int *__restrict__ counts, int64_t R, int64_t base,
                                                               int64_t *offs, int64_t *indptr_out) {
    __shared__ int64_t part[kKnnBlock];
    const int64_t seg = (R + kKnnBlock - 1) / kKnnBlock;
    const int64_t lo = (int64_t)threadIdx.x * seg < R ? (int64_t)threadIdx.x * seg : R, hi = lo + seg < R ? lo + seg : R;
    int64_t s = 0;
    for (int64_t j = lo; j < hi; ++j) s += counts[j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < kKnnBlock; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
        }
        offs[R] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t j = lo; j < hi; ++j) {
        offs[j] = run;
        run += counts[j];
        indptr_out[j + 1] = base + run;
    }
}

// the non-zero quotients of pass row b, ascending column, to idx / val at offs[b]
__global__ __launch_bounds__(kKnnBlock) void knn_compact_kernel(const double *__restrict__ S_all, int64_t n_rows,
                                                                const int64_t *__restrict__ offs, int32_t *idx, double *val) {
    const int64_t b = blockIdx.x;
    const double *S = S_all + b * n_rows;
    __shared__ int wsum[kKnnBlock / kKnnWave];
    const int lane = threadIdx.x & (kKnnWave - 1), wave = threadIdx.x / kKnnWave;
    int64_t out = offs[b];
    for (int64_t i0 = 0; i0 < n_rows; i0 += kKnnBlock) {
        const int64_t i = i0 + threadIdx.x;
        const double q = i < n_rows ? S[i] : 0.0;
        const bool keep = q != 0.0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int t = 0; t < kKnnBlock / kKnnWave; ++t) {
            if (t < wave) before += wsum[t];
            total += wsum[t];
        }
        if (keep) {
            const int64_t dst = out + before + __popcll(m & ((1ull << lane) - 1ull));
            idx[dst] = (int32_t)i;
            val[dst] = q;
        }
        out += total;
        __syncthreads();
    }
}

// ---- scoring -------------------------------------------------------------------------------------------------------------
// v[b, :] = 0, then Q's row of user rows[b] scattered into it (stored zeros stay zeros: they are no candidates)
__global__ void knn_dense_rows_kernel(const int64_t *__restrict__ q_ptr, const int32_t *__restrict__ q_idx,
                                      const double *__restrict__ q_val, const int32_t *__restrict__ rows, int64_t n_nb, double *v) {
    const int64_t b = blockIdx.x;
    const int32_t u = rows[b];
    double *dst = v + b * n_nb;
    for (int64_t i = threadIdx.x; i < n_nb; i += blockDim.x) dst[i] = 0.0;
    __syncthreads();
    for (int64_t e = q_ptr[u] + threadIdx.x; e < q_ptr[u + 1]; e += blockDim.x) dst[q_idx[e]] = q_val[e];
}

// doubles ordered as unsigned integers (-0.0 counts as +0.0, like the comparison of the values)
__device__ __forceinline__ unsigned long long knn_key(double w) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(w + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double knn_unkey(unsigned long long key) {
    return __longlong_as_double((long long)((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key));
}

__device__ __forceinline__ double knn_wave_sum(double v) {
    for (int o = kKnnWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kKnnWave);
    return v;
}

// One wave per task; task t scores item (items ? items[t] : t % n_items) for the dense row (items ? t : t / n_items).
// cand_w / cand_s: max_row doubles per workgroup.
__global__ __launch_bounds__(kKnnWave) void knn_score_kernel(
    const int64_t *__restrict__ n_ptr, const int32_t *__restrict__ n_idx, const double *__restrict__ n_val,
    const double *__restrict__ v_all, int64_t n_nb, int64_t n_items, const int32_t *__restrict__ items, int64_t n_tasks, int k,
    int user_mode, int64_t max_row, double *cand_w_all, double *cand_s_all, double *out) {
    __shared__ int hist[256];
    __shared__ int sel[2];
    __shared__ double tie[kKnnWave];
    const int lane = threadIdx.x;
    double *cw = cand_w_all + (int64_t)blockIdx.x * max_row, *cs = cand_s_all + (int64_t)blockIdx.x * max_row;
    for (int64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {   // (uniform per workgroup)
        const int64_t item = items ? (int64_t)items[t] : t % n_items;
        const double *v = v_all + (items ? t : t / n_items) * n_nb;
        const int64_t p0 = n_ptr[item], len = n_ptr[item + 1] - p0;
        // the candidates, in feed order: the row from its last entry to its first
        int64_t C = 0;
        for (int64_t q0 = 0; q0 < len; q0 += kKnnWave) {
            const int64_t q = q0 + lane;
            double w = 0.0, s = 0.0;
            bool is = false;
            if (q < len) {
                const int64_t e = p0 + len - 1 - q;
                const double x = v[n_idx[e]], sv = n_val[e];
                is = x != 0.0;
                w = user_mode ? x : sv;
                s = user_mode ? sv : x;
            }
            const unsigned long long m = __ballot(is);
            if (is) {
                const int64_t dst = C + __popcll(m & ((1ull << lane) - 1ull));
                cw[dst] = w;
                cs[dst] = s;
            }
            C += __popcll(m);
        }
        __syncthreads();   // (one wave: orders the buffer's stores before its loads)
        double num = 0.0, den = 0.0;
        if (C <= k) {
            for (int64_t p = lane; p < C; p += kKnnWave) {
                const double w = cw[p];
                num += w * cs[p];
                den += fabs(w);
            }
        } else {
            // T = the k-th largest weight: most significant byte first; `remaining` is its rank among the keys that share
            // the prefix, `above` counts the keys known to be larger
            unsigned long long prefix = 0;
            int remaining = k;
            int64_t above = 0;
            for (int shift = 56; shift >= 0; shift -= 8) {
                for (int bin = lane; bin < 256; bin += kKnnWave) hist[bin] = 0;
                __syncthreads();
                for (int64_t p = lane; p < C; p += kKnnWave) {
                    const unsigned long long key = knn_key(cw[p]);
                    if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
                }
                __syncthreads();
                // lane L holds bins 255 - 4L .. 252 - 4L: an inclusive scan over the lanes runs from the largest digit down
                int c4[4], mine = 0;
                for (int j = 0; j < 4; ++j) {
                    c4[j] = hist[255 - 4 * lane - j];
                    mine += c4[j];
                }
                int incl = mine;
                for (int o = 1; o < kKnnWave; o <<= 1) {
                    const int up = __shfl_up(incl, o, kKnnWave);
                    if (lane >= o) incl += up;
                }
                const unsigned long long crossed = __ballot(incl >= remaining);   // (never empty: remaining <= matching keys)
                const int first = __ffsll((long long)crossed) - 1;
                if (lane == first) {
                    int before = incl - mine;
                    for (int j = 0; j < 4; ++j) {
                        if (before + c4[j] >= remaining) {
                            sel[0] = 255 - 4 * lane - j;
                            sel[1] = before;
                            break;
                        }
                        before += c4[j];
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | (unsigned long long)sel[0];
                remaining -= sel[1];
                above += sel[1];
                __syncthreads();   // (sel and hist are rewritten by the next round)
            }
            const unsigned long long key_t = prefix;
            // P = the first k candidates with weight >= T; its members at T go to `tie`, one per lane; the candidates above T
            // are all survivors and are summed here
            int64_t ge_seen = 0;
            int n_tie = 0, above_in_p = 0;
            for (int64_t q0 = 0; q0 < C; q0 += kKnnWave) {
                const int64_t p = q0 + lane;
                bool gt = false, eq = false;
                double w = 0.0, s = 0.0;
                if (p < C) {
                    w = cw[p];
                    s = cs[p];
                    const unsigned long long key = knn_key(w);
                    gt = key > key_t;
                    eq = key == key_t;
                }
                if (gt) {
                    num += w * s;
                    den += fabs(w);
                }
                const unsigned long long m_ge = __ballot(gt || eq);
                const int64_t my_rank = ge_seen + __popcll(m_ge & ((1ull << lane) - 1ull));
                const bool in_p = (gt || eq) && my_rank < k;
                const unsigned long long m_tie = __ballot(in_p && eq), m_gp = __ballot(in_p && gt);
                if (in_p && eq) tie[n_tie + __popcll(m_tie & ((1ull << lane) - 1ull))] = s;   // (< k <= 64 slots)
                n_tie += __popcll(m_tie);
                above_in_p += __popcll(m_gp);
                ge_seen += __popcll(m_ge);
            }
            __syncthreads();
            const double tw = knn_unkey(key_t);
            const int evict = (int)(above - above_in_p);   // candidates above T fed after P: each pushes out the smallest pair
            if (lane < n_tie) {
                const double mine = tie[lane];
                int rank = 0;
                for (int j = 0; j < n_tie; ++j) {
                    const double o = tie[j];
                    rank += (o < mine) || (o == mine && j < lane);
                }
                if (rank >= evict) {
                    num += tw * mine;
                    den += fabs(tw);
                }
            }
        }
        num = knn_wave_sum(num);
        den = knn_wave_sum(den);
        if (lane == 0) out[t] = num / (den + 1e-8);
        __syncthreads();   // (the buffers and `tie` are rewritten by the next task)
    }
}

}  // namespace
}  // namespace chip

using namespace chip;

// ---- similarity handle ---------------------------------------------------------------------------------------------------
struct KnnChunk {
    int64_t first = 0, count = 0;   // position in the result and number of entries
    DevBuf<int32_t> idx;
    DevBuf<double> val;
};

struct cornac_hip_knn_sim : ModelHandle {
    int64_t n_rows = 0, n_cols = 0, nnz_in = 0;
    DevCsr rows, cols;   // W and its transpose
    DevBuf<int64_t> indptr, offs;
    DevBuf<double> S, D1, D2;
    DevBuf<int> counts;
    std::vector<std::unique_ptr<KnnChunk>> chunks;
    int64_t nnz_out = -1;   // -1: not run yet
};

int cornac_hip_knn_sim_create(cornac_hip_knn_sim_t *out, int device, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                              const int32_t *indices, const double *data) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_rows > 0 && n_cols > 0, "KNN: sizes must be positive");
        REQUIRE(n_rows < (1ll << 31) && n_cols < (1ll << 31), "KNN: row and column counts must fit int32");
        check_csr("KNN", "W", n_rows, n_cols, indptr, indices, data, kCsrValues);
        // the columns' entries, rows ascending (what data_mat.T.tocsr() holds, similarity.pyx:55)
        const HostCsr t = transpose_csr(n_rows, n_cols, indptr, indices, data);
        std::unique_ptr<cornac_hip_knn_sim> h(new cornac_hip_knn_sim());
        h->open(device);
        h->n_rows = n_rows; h->n_cols = n_cols; h->nnz_in = indptr[n_rows];
        h->rows.upload("KNN", "W", n_rows, indptr, indices, data, h->stream);
        h->cols.upload("KNN", "W transposed", t, h->stream);
        alloc_named(h->indptr, (size_t)n_rows + 1, "KNN", "the result's row pointers");
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_knn_sim_destroy(cornac_hip_knn_sim_t h) { return destroy_handle(h); }

int cornac_hip_knn_sim_run(cornac_hip_knn_sim_t h, int64_t rows_per_pass) {
    return guarded([&] {
        check_handle(h, "KNN similarity handle");
        REQUIRE(rows_per_pass >= 0, "KNN: rows_per_pass must be >= 0 (0: chosen from the free device memory)");
        const int64_t n = h->n_rows;
        int64_t R = rows_per_pass;
        if (R == 0) {
            // per pass row: three accumulators of n doubles and at most n (int32, double) result entries; use up to half of
            // what is free
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            const size_t per_row = (size_t)n * (3 * sizeof(double) + sizeof(double) + sizeof(int32_t));
            R = (int64_t)((free_b / 2) / per_row);
            if (R < 1)
                fail(CORNAC_HIP_ERR_HIP, "KNN: %zu bytes of free device memory do not hold the accumulators of one row (%zu bytes)",
                     free_b, per_row);
        }
        R = std::min<int64_t>(std::min(R, n), 1 << 20);
        h->chunks.clear();
        h->nnz_out = -1;
        alloc_named(h->S, (size_t)R * n, "KNN", "the similarity accumulators (lower rows_per_pass)");
        alloc_named(h->D1, (size_t)R * n, "KNN", "the similarity accumulators (lower rows_per_pass)");
        alloc_named(h->D2, (size_t)R * n, "KNN", "the similarity accumulators (lower rows_per_pass)");
        alloc_named(h->counts, (size_t)R, "KNN", "the row counts");
        alloc_named(h->offs, (size_t)R + 1, "KNN", "the row offsets");
        HIP_CHECK(hipMemsetAsync(h->indptr.p, 0, sizeof(int64_t), h->stream));
        int64_t total = 0;
        for (int64_t r0 = 0; r0 < n; r0 += R) {
            const int64_t rows = std::min(R, n - r0);
            knn_sim_rows_kernel<<<dim3((unsigned)rows), kKnnBlock, 0, h->stream>>>(
                h->rows.ptr.p, h->rows.idx.p, h->rows.val.p, h->cols.ptr.p, h->cols.idx.p, h->cols.val.p, n, r0, h->S.p, h->D1.p,
                h->D2.p, h->counts.p);
            knn_prefix_kernel<<<1, kKnnBlock, 0, h->stream>>>(h->counts.p, rows, total, h->offs.p, h->indptr.p + r0);
            HIP_CHECK(hipGetLastError());
            int64_t count = 0;
            HIP_CHECK(hipMemcpyAsync(&count, h->offs.p + rows, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
            REQUIRE(count >= 0 && count <= rows * n, "KNN: the device counted %lld entries for %lld rows", (long long)count,
                    (long long)rows);
            std::unique_ptr<KnnChunk> ch(new KnnChunk());
            ch->first = total;
            ch->count = count;
            if (count) {
                alloc_named(ch->idx, (size_t)count, "KNN", "the similarity table's indices");
                alloc_named(ch->val, (size_t)count, "KNN", "the similarity table's values");
                knn_compact_kernel<<<dim3((unsigned)rows), kKnnBlock, 0, h->stream>>>(h->S.p, n, h->offs.p, ch->idx.p, ch->val.p);
                HIP_CHECK(hipGetLastError());
            }
            h->chunks.push_back(std::move(ch));
            total += count;
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        for (DevBuf<double> *b : {&h->S, &h->D1, &h->D2}) b->release();
        h->nnz_out = total;
    });
}

int cornac_hip_knn_sim_nnz(cornac_hip_knn_sim_t h, int64_t *nnz) {
    return guarded([&] {
        check_handle(h, "KNN similarity handle");
        REQUIRE(nnz != nullptr, "nnz pointer is NULL");
        REQUIRE(h->nnz_out >= 0, "KNN: the similarity has not been run");
        *nnz = h->nnz_out;
    });
}

int cornac_hip_knn_sim_get(cornac_hip_knn_sim_t h, int64_t *indptr, int32_t *indices, double *data) {
    return guarded([&] {
        check_handle(h, "KNN similarity handle");
        REQUIRE(h->nnz_out >= 0, "KNN: the similarity has not been run");
        REQUIRE(indptr && (h->nnz_out == 0 || (indices && data)), "KNN: result pointers are NULL");
        h->indptr.download(indptr, (size_t)h->n_rows + 1, h->stream);
        for (const auto &ch : h->chunks)
            if (ch->count) {
                ch->idx.download(indices + ch->first, (size_t)ch->count, h->stream);
                ch->val.download(data + ch->first, (size_t)ch->count, h->stream);
            }
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

// ---- scorer handle -------------------------------------------------------------------------------------------------------
struct cornac_hip_knn_scorer : ModelHandle {
    int user_mode = 0;
    int64_t n_items = 0, n_nb = 0, n_users = 0, max_row = 0;
    DevCsr N, Q;
    DevBuf<double> v, cand_w, cand_s, out;
    int blocks = 0;
};

int cornac_hip_knn_scorer_create(cornac_hip_knn_scorer_t *out, int device, int64_t n_items, int64_t n_neighbours,
                                 int64_t n_users, const int64_t *n_indptr, const int32_t *n_indices, const double *n_data,
                                 const int64_t *q_indptr, const int32_t *q_indices, const double *q_data, int user_mode) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_items > 0 && n_neighbours > 0 && n_users > 0, "KNN: sizes must be positive");
        REQUIRE(n_items < (1ll << 31) && n_neighbours < (1ll << 31) && n_users < (1ll << 31), "KNN: sizes must fit int32");
        check_csr("KNN", "N", n_items, n_neighbours, n_indptr, n_indices, n_data, kCsrValues);
        check_csr("KNN", "Q", n_users, n_neighbours, q_indptr, q_indices, q_data, kCsrValues);
        std::unique_ptr<cornac_hip_knn_scorer> h(new cornac_hip_knn_scorer());
        h->open(device);
        h->user_mode = user_mode != 0;
        h->n_items = n_items; h->n_nb = n_neighbours; h->n_users = n_users;
        for (int64_t i = 0; i < n_items; ++i) h->max_row = std::max(h->max_row, n_indptr[i + 1] - n_indptr[i]);
        h->N.upload("KNN", "N", n_items, n_indptr, n_indices, n_data, h->stream);
        h->Q.upload("KNN", "Q", n_users, q_indptr, q_indices, q_data, h->stream);
        // one candidate buffer of max_row (weight, rating) pairs per resident workgroup: at most 1 GiB of them
        const int64_t per_block = std::max<int64_t>(h->max_row, 1) * 2 * (int64_t)sizeof(double);
        h->blocks = (int)std::max<int64_t>(1, std::min<int64_t>(8192, (1ll << 30) / per_block));
        alloc_named(h->cand_w, (size_t)h->blocks * (size_t)std::max<int64_t>(h->max_row, 1), "KNN", "the candidate buffers");
        alloc_named(h->cand_s, (size_t)h->blocks * (size_t)std::max<int64_t>(h->max_row, 1), "KNN", "the candidate buffers");
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_knn_scorer_destroy(cornac_hip_knn_scorer_t h) { return destroy_handle(h); }

// users[0..n) (and items[0..n) for pairs) in chunks whose dense rows of Q take at most kKnnDenseBytes
static void knn_score(cornac_hip_knn_scorer_t h, const int32_t *users, const int32_t *items, int64_t n, int k, double *out) {
    check_handle(h, "KNN scorer handle");
    REQUIRE(k >= 1 && k <= kKnnMaxK, "KNN: k = %d is outside 1 .. %d (CORNAC_HIP_KNN_MAX_K)", k, kKnnMaxK);
    check_ids("KNN", users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t per_task_row = items ? 1 : h->n_items;
    const int64_t B = std::max<int64_t>(1, std::min<int64_t>(n, kKnnDenseBytes / ((int64_t)sizeof(double) * h->n_nb)));
    if (h->v.n < (size_t)(B * h->n_nb)) alloc_named(h->v, (size_t)(B * h->n_nb), "KNN", "the users' dense rows");
    if (h->out.n < (size_t)(B * per_task_row)) alloc_named(h->out, (size_t)(B * per_task_row), "KNN", "the scores");
    for_each_chunk("KNN", *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        const int64_t tasks = nb * per_task_row;
        knn_dense_rows_kernel<<<dim3((unsigned)nb), kKnnBlock, 0, h->stream>>>(h->Q.ptr.p, h->Q.idx.p, h->Q.val.p, h->user_ids.p,
                                                                              h->n_nb, h->v.p);
        const unsigned grid = (unsigned)std::min<int64_t>(tasks, h->blocks);
        knn_score_kernel<<<dim3(grid), kKnnWave, 0, h->stream>>>(h->N.ptr.p, h->N.idx.p, h->N.val.p, h->v.p, h->n_nb, h->n_items,
                                                                 items ? h->item_ids.p : nullptr, tasks, k, h->user_mode, h->max_row,
                                                                 h->cand_w.p, h->cand_s.p, h->out.p);
        h->out.download(out + b0 * per_task_row, (size_t)tasks, h->stream);
    });
}

int cornac_hip_knn_scorer_score_users(cornac_hip_knn_scorer_t h, const int32_t *users, int64_t n, int k, double *out) {
    return guarded([&] { knn_score(h, users, nullptr, n, k, out); });
}

int cornac_hip_knn_scorer_score_pairs(cornac_hip_knn_scorer_t h, const int32_t *users, const int32_t *items, int64_t n, int k,
                                      double *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "KNN: items is NULL");
        knn_score(h, users, items, n, k, out);
    });
}

// Host scaffold of the models that score from a device handle of their own: named device allocation, CSR validation /
// transpose / upload, the handle's device and stream, the map from a named table to its place in a device buffer with the one
// copy path of set_params / get_params / get_state and the reset of the optimiser state, and the id-checked chunk loop of
// their score_users / score_pairs entry points.  Included by knn.hip and ease.hip, and through vae_host.h by vaecf.hip, bivae.hip,
// recvae.hip, ncf.hip and graph.h (lightgcn.hip, ngcf.hip).  Host code only; every message carries the model's prefix.
#pragma once
#include "common.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace chip {

// b <- count elements; a refusal names the model and what the memory was for
template <class T>
void alloc_named(DevBuf<T> &b, size_t count, const char *model, const char *what) {
    b.release();
    if (!count) return;
    T *p = nullptr;
    const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(CORNAC_HIP_ERR_HIP, "%s: cannot allocate %zu bytes of device memory for %s (%s)", model, count * sizeof(T), what,
             hipGetErrorString(e));
    }
    b.p = p;
    b.n = count;
}

enum CsrValues { kCsrNoValues, kCsrValues, kCsrFiniteValues };

// indptr starts at 0 and is monotone; the indices are in range, sorted and without repeats; the values are there (and finite)
// where `values` asks for them.  Needs no device.
inline void check_csr(const char *model, const char *name, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                      const int32_t *indices, const double *data, CsrValues values) {
    REQUIRE(indptr != nullptr, "%s: %s indptr is NULL", model, name);
    REQUIRE(indptr[0] == 0, "%s: %s indptr does not start at 0", model, name);
    for (int64_t r = 0; r < n_rows; ++r) REQUIRE(indptr[r] <= indptr[r + 1], "%s: %s indptr is not monotone", model, name);
    const int64_t nnz = indptr[n_rows];
    REQUIRE(nnz == 0 || (indices && (data || values == kCsrNoValues)), "%s: %s indices / data are NULL", model, name);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            REQUIRE(indices[e] >= 0 && indices[e] < n_cols, "%s: %s column index out of range in row %lld", model, name,
                    (long long)r);
            REQUIRE(e == indptr[r] || indices[e - 1] < indices[e], "%s: %s needs sorted indices without repeats (row %lld)",
                    model, name, (long long)r);
            REQUIRE(values != kCsrFiniteValues || std::isfinite(data[e]), "%s: the value of %s in row %lld, column %d is not finite",
                    model, name, (long long)r, indices[e]);
        }
}

struct HostCsr {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    std::vector<double> val;
};

// the columns' entries, rows ascending (what scipy's mat.T.tocsr() holds): a counting sort; data may be NULL (no values)
inline HostCsr transpose_csr(int64_t n_rows, int64_t n_cols, const int64_t *indptr, const int32_t *indices, const double *data) {
    const int64_t nnz = indptr[n_rows];
    HostCsr t;
    t.ptr.assign((size_t)n_cols + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) ++t.ptr[(size_t)indices[e] + 1];
    for (int64_t c = 0; c < n_cols; ++c) t.ptr[(size_t)c + 1] += t.ptr[(size_t)c];
    t.idx.resize((size_t)nnz);
    if (data) t.val.resize((size_t)nnz);
    std::vector<int64_t> fill(t.ptr.begin(), t.ptr.end() - 1);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            const int64_t d = fill[(size_t)indices[e]]++;
            t.idx[(size_t)d] = (int32_t)r;
            if (data) t.val[(size_t)d] = data[e];
        }
    return t;
}

// a CSR matrix on the device; val stays empty for a matrix without values
struct DevCsr {
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> idx;
    DevBuf<double> val;
    // allocate and enqueue the copies on `stream`; the host arrays must live until the stream is synchronised
    void upload(const char *model, const char *name, int64_t n_rows, const int64_t *indptr, const int32_t *indices,
                const double *data, hipStream_t stream) {
        const size_t nnz = (size_t)indptr[n_rows];
        const std::string what = std::string(name) + "'s pointers, indices and values";
        alloc_named(ptr, (size_t)n_rows + 1, model, what.c_str());
        alloc_named(idx, nnz, model, what.c_str());
        if (data) alloc_named(val, nnz, model, what.c_str());
        ptr.upload(indptr, (size_t)n_rows + 1, stream);
        if (nnz) idx.upload(indices, nnz, stream);
        if (nnz && data) val.upload(data, nnz, stream);
    }
    void upload(const char *model, const char *name, const HostCsr &m, hipStream_t stream) {
        upload(model, name, (int64_t)m.ptr.size() - 1, m.ptr.data(), m.idx.data(), m.val.empty() ? nullptr : m.val.data(), stream);
    }
};

// what every handle of these models starts with: its device, its stream and the id buffers of the chunk loop
struct ModelHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf<int32_t> user_ids, item_ids;
    // after the arguments are validated: makes `device` current (a gfx950 part) and creates the stream
    void open(int dev) {
        use_device(dev);
        device = dev;
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
};

inline void check_handle(const ModelHandle *h, const char *what) {
    REQUIRE(h != nullptr, "%s is NULL", what);
    HIP_CHECK(hipSetDevice(h->device));
}

// H: the model's handle struct, derived from ModelHandle (deleted as what it is: no virtual destructor)
template <class H>
int destroy_handle(H *h) {
    if (!h) return CORNAC_HIP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    delete h;
    return CORNAC_HIP_OK;
}

// One named table of a handle model: where it starts in a device buffer (the parameters, or an optimiser-state buffer of the
// same layout) and its shape on the host, rows x cols.  transposed: the device holds it [cols x rows] (a first layer's weight,
// one row per input id).  A handle lists its tables once, in create, in the reference's state_dict order.
struct TableSlot {
    int64_t off, rows, cols;
    bool transposed;
};

// dst [cols x rows] <- the transpose of src [rows x cols]
inline void transpose_table(const float *src, int64_t rows, int64_t cols, float *dst) {
    for (int64_t j = 0; j < rows; ++j)
        for (int64_t i = 0; i < cols; ++i) dst[i * rows + j] = src[j * cols + i];
}

// host -> device copy of the tables of `slots` into the buffer at `base`; host[q] is slot q's table in the host's shape, and a
// NULL entry skips it.  Returns with every copy done: one wait, until which the transposed tables' staging lives.
inline void put_tables(hipStream_t stream, float *base, const std::vector<TableSlot> &slots, const float *const *host) {
    std::vector<std::vector<float>> staged;
    for (size_t q = 0; q < slots.size(); ++q) {
        if (!host[q]) continue;
        const TableSlot &s = slots[q];
        const float *src = host[q];
        if (s.transposed) {
            staged.emplace_back((size_t)(s.rows * s.cols));
            transpose_table(src, s.rows, s.cols, staged.back().data());
            src = staged.back().data();
        }
        HIP_CHECK(hipMemcpyAsync(base + s.off, src, (size_t)(s.rows * s.cols) * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
}

// device -> host, the same way: the transposed tables are turned once the one wait is over
inline void get_tables(hipStream_t stream, const float *base, const std::vector<TableSlot> &slots, float *const *host) {
    std::vector<std::vector<float>> staged(slots.size());
    for (size_t q = 0; q < slots.size(); ++q) {
        if (!host[q]) continue;
        const TableSlot &s = slots[q];
        float *dst = host[q];
        if (s.transposed) {
            staged[q].resize((size_t)(s.rows * s.cols));
            dst = staged[q].data();
        }
        HIP_CHECK(hipMemcpyAsync(dst, base + s.off, (size_t)(s.rows * s.cols) * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t q = 0; q < slots.size(); ++q)
        if (host[q] && slots[q].transposed) transpose_table(staged[q].data(), slots[q].cols, slots[q].rows, host[q]);
}

// reset_optimizer's device half: the optimiser-state buffers back to zero, done on return (the step counters are the caller's)
inline void zero_state(hipStream_t stream, std::initializer_list<DevBuf<float> *> buffers) {
    for (DevBuf<float> *b : buffers) HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// the arguments of score_users (items == NULL) / score_pairs against the handle's sizes
inline void check_ids(const char *model, const int32_t *users, const int32_t *items, int64_t n, const void *out, int64_t n_users,
                      int64_t n_items) {
    REQUIRE(n >= 0 && (n == 0 || (users && out)), "%s: users / out are NULL", model);
    for (int64_t b = 0; b < n; ++b) {
        REQUIRE(users[b] >= 0 && users[b] < n_users, "%s: user %d out of range", model, users[b]);
        REQUIRE(!items || (items[b] >= 0 && items[b] < n_items), "%s: item %d out of range", model, items ? items[b] : 0);
    }
}

// [0, n) in chunks of B ids: the chunk's ids go to h.user_ids (and h.item_ids), launch(b0, nb) enqueues its kernels and the
// download of its results, and the stream is synchronised before the next chunk reuses the buffers
template <class Launch>
void for_each_chunk(const char *model, ModelHandle &h, const int32_t *users, const int32_t *items, int64_t n, int64_t B,
                    Launch &&launch) {
    if (h.user_ids.n < (size_t)B) alloc_named(h.user_ids, (size_t)B, model, "the user ids");
    if (items && h.item_ids.n < (size_t)B) alloc_named(h.item_ids, (size_t)B, model, "the item ids");
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t nb = std::min(B, n - b0);
        h.user_ids.upload(users + b0, (size_t)nb, h.stream);
        if (items) h.item_ids.upload(items + b0, (size_t)nb, h.stream);
        launch(b0, nb);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(h.stream));
    }
}

}  // namespace chip

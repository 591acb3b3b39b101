// EASE (Steck 2019; cornac/models/ease/recom_ease.py:72-126) on gfx950, all in float64: the item-item weights
//   G = X^T X,  G_ii += lamb,  P = inv(G),  B = P / (-diag(P)) by columns,  B_ii = 0,  (posB) B[B < 0] = 0
// and the scores X[u, :] . B.  One handle owns X on the device (CSR and CSC) and ONE dense n_items x n_items table that is
// G, then P, then B, in place.  Every index into the table is 64-bit.
//
// Gram.  One workgroup owns row i of the table as its dense accumulator.  It walks item i's users in ascending order; the
// threads share the user's row of X (one target each: a row holds an item at most once) and a workgroup barrier separates
// two users, so every G[i, j] is summed over the users in ascending order, each *, + rounded on its own (the tree is
// built with -ffp-contract=off).  That is the order of SciPy's sparse product.  No float atomics.
//
// Inverse.  Blocked Gauss-Jordan without pivoting, block 64, in place (the table plus lamb I is SPD, and so is every
// pivot block: a Schur complement of an SPD matrix).  Per block k, with D = inv(A_kk):
//   pivot      one workgroup inverts A_kk in LDS by scalar Gauss-Jordan and leaves D in A_kk and in a 64 x 64 side buffer;
//   row panel  A_kj <- D A_kj                     (j != k)
//   update     A_ij <- A_ij - A_ik A_kj           (i != k, j != k): all the flops; 64 x 128 tiles, 4 x 8 outputs per
//              thread held in registers, the two panels staged through LDS 16 columns at a time, explicit fma chains in
//              ascending k (the update writes neither panel, so it needs no copy of them)
//   col panel  A_ik <- -(A_ik D)                  (i != k)
// Every sum has one fixed order.  A pivot that is not a positive finite number stores the block's number into a flag (an
// ordinary store of an int, first block wins); nothing aborts, and the call returns a status once the sweep is through.
//
// Scoring.  One thread per (user, output item), consecutive threads on consecutive items, so the rows of B are read
// coalesced: y = 0, then y += x * B[j, :] over the user's entries in ascending item order, * and + rounded on their own:
// the order of SciPy's csr . dense, for the full row and for the single column.
#include "sparse_model.h"

namespace chip {
namespace {

constexpr int kEaseBlock = 256;
constexpr int kEaseNb = 64;      // the Gauss-Jordan block
constexpr int kEaseTileM = 64;   // the update's output tile per workgroup: rows ...
constexpr int kEaseTileN = 128;  // ... and columns
constexpr int kEaseKc = 16;      // panel columns staged per round
static_assert(kEaseBlock == 4 * kEaseNb && kEaseTileM == kEaseNb && kEaseNb % kEaseKc == 0, "thread maps below");
static_assert(kEaseBlock == (kEaseTileM / 4) * (kEaseTileN / 8) && (kEaseKc * kEaseTileM) % kEaseBlock == 0,
              "the update's 4 x 8 outputs per thread");

// scoring chunks: at most kEaseScoreBytes of scores and kEaseMaxUsers users (the grid's y) per users call
constexpr int64_t kEaseScoreBytes = 256ll << 20, kEaseMaxUsers = 65535, kEaseMaxPairs = 1 << 20;

// ---- Gram ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEaseBlock) void ease_gram_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, const double *__restrict__ row_val,
    const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ col_idx, const double *__restrict__ col_val, int64_t n,
    double *G) {
    const int64_t i = blockIdx.x;
    double *row = G + i * n;
    for (int64_t j = threadIdx.x; j < n; j += kEaseBlock) row[j] = 0.0;
    __syncthreads();
    for (int64_t e = col_ptr[i]; e < col_ptr[i + 1]; ++e) {   // (uniform: every thread walks the item's users)
        const int32_t u = col_idx[e];
        const double w = col_val[e];
        for (int64_t q = row_ptr[u] + threadIdx.x; q < row_ptr[u + 1]; q += kEaseBlock) row[row_idx[q]] += w * row_val[q];
        __syncthreads();   // the next user may hit the same targets: its additions come after these
    }
}

__global__ void ease_add_diagonal_kernel(double *A, int64_t n, double lamb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[i * n + i] += lamb;
}

// ---- inverse -------------------------------------------------------------------------------------------------------------
// A_kk (m x m at (k0, k0)) <- its inverse, also to D[64 x 64] (zero outside m x m).  Thread (c = tid % 64, tid / 64) owns
// column c of rows tid / 64 + 4 q.
__global__ __launch_bounds__(kEaseBlock) void ease_pivot_kernel(double *A, int64_t n, int64_t k0, int m, double *D, int *flag,
                                                                int block_no) {
    __shared__ double a[kEaseNb][kEaseNb + 1];
    const int c = threadIdx.x % kEaseNb, r0 = threadIdx.x / kEaseNb;
    for (int q = 0; q < 16; ++q) {
        const int r = r0 + 4 * q;
        a[r][c] = (r < m && c < m) ? A[(k0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    bool bad = false;
    for (int t = 0; t < m; ++t) {
        const double p = a[t][t];
        bad = bad || !(p > 0.0) || !(p < INFINITY);
        const double inv = 1.0 / p, rt = a[t][c] * inv;
        double f[16];
        for (int q = 0; q < 16; ++q) f[q] = a[r0 + 4 * q][t];
        __syncthreads();   // every read of row t and column t comes before their rewriting
        for (int q = 0; q < 16; ++q) {
            const int r = r0 + 4 * q;
            double v;
            if (r == t) v = c == t ? inv : rt;
            else if (c == t) v = -(f[q] * inv);
            else v = a[r][c] - f[q] * rt;
            a[r][c] = v;
        }
        __syncthreads();
    }
    for (int q = 0; q < 16; ++q) {
        const int r = r0 + 4 * q;
        const bool in = r < m && c < m;
        const double v = in ? a[r][c] : 0.0;
        D[r * kEaseNb + c] = v;
        if (in) A[(k0 + r) * n + k0 + c] = v;
    }
    if (threadIdx.x == 0 && bad && *flag == 0) *flag = block_no + 1;   // (launches of one stream: the first block stays)
}

// A_kj <- D A_kj for the 64 columns at blockIdx.x * 64 (the pivot's own columns are left alone)
__global__ __launch_bounds__(kEaseBlock) void ease_row_panel_kernel(double *A, int64_t n, int64_t k0, int m,
                                                                    const double *__restrict__ D) {
    const int64_t j0 = (int64_t)blockIdx.x * kEaseNb;
    if (j0 == k0) return;
    __shared__ double T[kEaseNb][kEaseNb];
    const int c = threadIdx.x % kEaseNb, w = threadIdx.x / kEaseNb;
    const int64_t j = j0 + c;
    for (int q = 0; q < 16; ++q) {
        const int r = w + 4 * q;
        T[r][c] = (r < m && j < n) ? A[(k0 + r) * n + j] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < 16; ++q) {
        const int r = w * 16 + q;   // (uniform per wave: D's row is one address for all of its lanes)
        double acc = 0.0;
        for (int t = 0; t < kEaseNb; ++t) acc = fma(D[r * kEaseNb + t], T[t][c], acc);
        if (r < m && j < n) A[(k0 + r) * n + j] = acc;
    }
}

// A_ik <- -(A_ik D) for the 64 rows at blockIdx.x * 64 (the pivot's own rows are left alone)
__global__ __launch_bounds__(kEaseBlock) void ease_col_panel_kernel(double *A, int64_t n, int64_t k0, int m,
                                                                    const double *__restrict__ D) {
    const int64_t i0 = (int64_t)blockIdx.x * kEaseNb;
    if (i0 == k0) return;
    __shared__ double T[kEaseNb][kEaseNb + 1];
    const int c = threadIdx.x % kEaseNb, w = threadIdx.x / kEaseNb;
    for (int q = 0; q < 16; ++q) {
        const int r = w + 4 * q;
        T[r][c] = (i0 + r < n && c < m) ? A[(i0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int q = 0; q < 16; ++q) {
        const int r = w * 16 + q;
        double acc = 0.0;
        for (int t = 0; t < kEaseNb; ++t) acc = fma(T[r][t], D[t * kEaseNb + c], acc);
        if (i0 + r < n && c < m) A[(i0 + r) * n + k0 + c] = -acc;
    }
}

// A_ij <- A_ij - sum_t A[i, k0 + t] A[k0 + t, j] over a 64 x 128 tile, rows and columns of the pivot block excluded: a
// tile's rows are one block, its columns two, so the exclusion is uniform per workgroup and per column half.
// Thread (tx = tid % 16, ty = tid / 16) holds the row pairs 2 ty + 32 a and the column pairs 2 tx + 32 b (a < 2, b < 4):
// 4 x 8 outputs, few enough registers for several workgroups per CU, whose loads and stores of C then overlap with each
// other's arithmetic; pairs, so that the LDS reads are 16 bytes wide.  Every element sits at a uniform base plus a
// 32-bit offset of the thread's own (63 n + 127 doubles at most: the host refuses an n at which that would not fit).
__global__ __launch_bounds__(kEaseBlock) void ease_update_kernel(double *A, int64_t n, int64_t k0, int m) {
    __shared__ __attribute__((aligned(16))) double sL[kEaseKc][kEaseTileM + 2];
    __shared__ __attribute__((aligned(16))) double sR[kEaseKc][kEaseTileN];
    const int64_t i0 = (int64_t)blockIdx.y * kEaseTileM, j0 = (int64_t)blockIdx.x * kEaseTileN;
    if (i0 == k0) return;   // (uniform) the row panel itself
    const bool skip_lo = j0 == k0, skip_hi = j0 + kEaseNb == k0;
    const int rows = (int)(n - i0 < kEaseTileM ? n - i0 : kEaseTileM), cols = (int)(n - j0 < kEaseTileN ? n - j0 : kEaseTileN);
    const uint32_t ld = (uint32_t)n;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const int r0 = 2 * ty, c0 = 2 * tx;
    char *const tile = reinterpret_cast<char *>(A + i0 * n + j0);
    const uint32_t own = ((uint32_t)r0 * ld + (uint32_t)c0) * (uint32_t)sizeof(double);
    double acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int da = 32 * (a >> 1) + (a & 1);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int db = 32 * (b >> 1) + (b & 1);
            const uint32_t off = own + ((uint32_t)da * ld + (uint32_t)db) * (uint32_t)sizeof(double);
            acc[a][b] = (r0 + da < rows && c0 + db < cols) ? *reinterpret_cast<const double *>(tile + off) : 0.0;
        }
    }
#pragma unroll 1
    for (int t0 = 0; t0 < kEaseNb; t0 += kEaseKc) {
        const char *const lbase = reinterpret_cast<const char *>(A + i0 * n + k0 + t0);
        const char *const rbase = reinterpret_cast<const char *>(A + (k0 + t0) * n + j0);
#pragma unroll
        for (int q = 0; q < kEaseKc * kEaseTileM / kEaseBlock; ++q) {
            const int idx = threadIdx.x + kEaseBlock * q;
            const int r = idx / kEaseKc, t = idx % kEaseKc;
            const uint32_t off = ((uint32_t)r * ld + (uint32_t)t) * (uint32_t)sizeof(double);
            sL[t][r] = (r < rows && t0 + t < m) ? *reinterpret_cast<const double *>(lbase + off) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kEaseKc * kEaseTileN / kEaseBlock; ++q) {
            const int idx = threadIdx.x + kEaseBlock * q;
            const int t = idx / kEaseTileN, c = idx % kEaseTileN;
            const uint32_t off = ((uint32_t)t * ld + (uint32_t)c) * (uint32_t)sizeof(double);
            sR[t][c] = (c < cols && t0 + t < m) ? *reinterpret_cast<const double *>(rbase + off) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kEaseKc; ++t) {
            double l[4], r[8];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const double2 v = *reinterpret_cast<const double2 *>(&sL[t][r0 + 32 * a]);
                l[2 * a] = -v.x;
                l[2 * a + 1] = -v.y;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double2 v = *reinterpret_cast<const double2 *>(&sR[t][c0 + 32 * b]);
                r[2 * b] = v.x;
                r[2 * b + 1] = v.y;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = fma(l[a], r[b], acc[a][b]);
        }
        __syncthreads();   // (the staging buffers are rewritten by the next round)
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int da = 32 * (a >> 1) + (a & 1);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int db = 32 * (b >> 1) + (b & 1);
            const uint32_t off = own + ((uint32_t)da * ld + (uint32_t)db) * (uint32_t)sizeof(double);
            if (r0 + da < rows && c0 + db < cols && !(db < kEaseNb ? skip_lo : skip_hi)) *reinterpret_cast<double *>(tile + off) = acc[a][b];
        }
    }
}

// ---- weights -------------------------------------------------------------------------------------------------------------
__global__ void ease_diagonal_kernel(const double *__restrict__ A, int64_t n, double *d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = A[i * n + i];
}

// B[i, j] = P[i, j] / (-P[j, j]), 0 on the diagonal; with pos_b every entry that is not above 0 becomes +0.0
__global__ void ease_weights_kernel(double *A, int64_t n, const double *__restrict__ d, int pos_b) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double den = -d[j];
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        double b = A[i * n + j] / den;
        if (i == j) b = 0.0;
        if (pos_b && b <= 0.0) b = 0.0;
        A[i * n + j] = b;
    }
}

// ---- scoring -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEaseBlock) void ease_score_users_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx, const double *__restrict__ row_val,
    const int32_t *__restrict__ users, const double *__restrict__ B, int64_t n, double *out) {
    const int64_t j = (int64_t)blockIdx.x * kEaseBlock + threadIdx.x, b = blockIdx.y;
    if (j >= n) return;
    const int32_t u = users[b];
    double y = 0.0;
    for (int64_t e = row_ptr[u]; e < row_ptr[u + 1]; ++e) y += row_val[e] * B[(int64_t)row_idx[e] * n + j];
    out[b * n + j] = y;
}

__global__ void ease_score_pairs_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ row_idx,
                                        const double *__restrict__ row_val, const int32_t *__restrict__ users,
                                        const int32_t *__restrict__ items, const double *__restrict__ B, int64_t n,
                                        int64_t n_pairs, double *out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t u = users[p];
    const int64_t j = items[p];
    double y = 0.0;
    for (int64_t e = row_ptr[u]; e < row_ptr[u + 1]; ++e) y += row_val[e] * B[(int64_t)row_idx[e] * n + j];
    out[p] = y;
}

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_ease : ModelHandle {
    int64_t n_users = 0, n_items = 0;
    DevCsr rows, cols;   // X and its transpose
    DevBuf<double> table, diag, D, out;
    DevBuf<int> flag;
};

int cornac_hip_ease_create(cornac_hip_ease_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, const double *data) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "EASE: sizes must be positive");
        REQUIRE(n_users < (1ll << 31) && n_items < (1ll << 31), "EASE: user and item counts must fit int32");
        check_csr("EASE", "X", n_users, n_items, indptr, indices, data, kCsrFiniteValues);
        const HostCsr t = transpose_csr(n_users, n_items, indptr, indices, data);   // the items' entries, users ascending
        std::unique_ptr<cornac_hip_ease> h(new cornac_hip_ease());
        h->open(device);
        h->n_users = n_users; h->n_items = n_items;
        {
            // a table beyond the device's whole memory is refused before the allocator is asked
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            const size_t want = (size_t)n_items * (size_t)n_items * sizeof(double);
            if (want > total_b)
                fail(CORNAC_HIP_ERR_HIP, "EASE: cannot allocate %zu bytes of device memory for the item-item table (the device has %zu)",
                     want, total_b);
        }
        alloc_named(h->table, (size_t)n_items * (size_t)n_items, "EASE", "the item-item table");
        alloc_named(h->diag, (size_t)n_items, "EASE", "the diagonal");
        alloc_named(h->D, (size_t)kEaseNb * kEaseNb, "EASE", "the pivot block");
        alloc_named(h->flag, 1, "EASE", "the status flag");
        HIP_CHECK(hipMemsetAsync(h->table.p, 0, h->table.n * sizeof(double), h->stream));
        h->rows.upload("EASE", "X", n_users, indptr, indices, data, h->stream);
        h->cols.upload("EASE", "X transposed", t, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

int cornac_hip_ease_destroy(cornac_hip_ease_t h) { return destroy_handle(h); }

static void ease_gram(cornac_hip_ease_t h) {
    ease_gram_kernel<<<dim3((unsigned)h->n_items), kEaseBlock, 0, h->stream>>>(
        h->rows.ptr.p, h->rows.idx.p, h->rows.val.p, h->cols.ptr.p, h->cols.idx.p, h->cols.val.p, h->n_items, h->table.p);
    HIP_CHECK(hipGetLastError());
}

static void ease_invert(cornac_hip_ease_t h, double lamb) {
    REQUIRE(lamb > 0.0 && std::isfinite(lamb), "EASE: lamb must be a positive finite number, got %g", lamb);
    const int64_t n = h->n_items;
    double *A = h->table.p;
    HIP_CHECK(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
    ease_add_diagonal_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, h->stream>>>(A, n, lamb);
    const unsigned strips = (unsigned)((n + kEaseNb - 1) / kEaseNb), tiles = (unsigned)((n + kEaseTileN - 1) / kEaseTileN);
    REQUIRE(strips <= 65535 && n < (1ll << 22), "EASE: %lld items are more than the update's grid holds", (long long)n);
    for (int64_t k0 = 0, k = 0; k0 < n; k0 += kEaseNb, ++k) {
        const int m = (int)std::min<int64_t>(kEaseNb, n - k0);
        ease_pivot_kernel<<<1, kEaseBlock, 0, h->stream>>>(A, n, k0, m, h->D.p, h->flag.p, (int)k);
        ease_row_panel_kernel<<<strips, kEaseBlock, 0, h->stream>>>(A, n, k0, m, h->D.p);
        ease_update_kernel<<<dim3(tiles, strips), kEaseBlock, 0, h->stream>>>(A, n, k0, m);
        ease_col_panel_kernel<<<strips, kEaseBlock, 0, h->stream>>>(A, n, k0, m, h->D.p);
        HIP_CHECK(hipGetLastError());
    }
    int flag = 0;
    h->flag.download(&flag, 1, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (flag) fail(CORNAC_HIP_ERR_INVALID, "EASE: the table plus lamb = %g on its diagonal is not positive definite at block %d", lamb, flag - 1);
}

static void ease_weights(cornac_hip_ease_t h, int pos_b) {
    const int64_t n = h->n_items;
    const unsigned gx = (unsigned)((n + 255) / 256);
    ease_diagonal_kernel<<<gx, 256, 0, h->stream>>>(h->table.p, n, h->diag.p);   // first: the pass overwrites the diagonal
    ease_weights_kernel<<<dim3(gx, (unsigned)std::min<int64_t>(n, 4096)), 256, 0, h->stream>>>(h->table.p, n, h->diag.p,
                                                                                              pos_b != 0);
    HIP_CHECK(hipGetLastError());
}

int cornac_hip_ease_gram(cornac_hip_ease_t h) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        ease_gram(h);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ease_invert(cornac_hip_ease_t h, double lamb) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        ease_invert(h, lamb);
    });
}

int cornac_hip_ease_weights(cornac_hip_ease_t h, int pos_b) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        ease_weights(h, pos_b);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ease_fit(cornac_hip_ease_t h, double lamb, int pos_b) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        REQUIRE(lamb > 0.0 && std::isfinite(lamb), "EASE: lamb must be a positive finite number, got %g", lamb);
        ease_gram(h);
        ease_invert(h, lamb);
        ease_weights(h, pos_b);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ease_get_table(cornac_hip_ease_t h, double *table) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        REQUIRE(table != nullptr, "EASE: table pointer is NULL");
        h->table.download(table, h->table.n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

int cornac_hip_ease_set_table(cornac_hip_ease_t h, const double *table) {
    return guarded([&] {
        check_handle(h, "EASE handle");
        REQUIRE(table != nullptr, "EASE: table pointer is NULL");
        h->table.upload(table, h->table.n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

// users[0..n) (and items[0..n) for pairs) in chunks whose scores take at most kEaseScoreBytes on the device
static void ease_score(cornac_hip_ease_t h, const int32_t *users, const int32_t *items, int64_t n, double *out) {
    check_handle(h, "EASE handle");
    check_ids("EASE", users, items, n, out, h->n_users, h->n_items);
    if (n == 0) return;
    const int64_t ni = h->n_items, per_user = items ? 1 : ni;
    const int64_t cap = items ? kEaseMaxPairs
                              : std::min<int64_t>(kEaseMaxUsers, std::max<int64_t>(1, kEaseScoreBytes / ((int64_t)sizeof(double) * ni)));
    const int64_t B = std::min(n, cap);
    if (h->out.n < (size_t)(B * per_user)) alloc_named(h->out, (size_t)(B * per_user), "EASE", "the scores");
    for_each_chunk("EASE", *h, users, items, n, B, [&](int64_t b0, int64_t nb) {
        if (items) {
            ease_score_pairs_kernel<<<dim3((unsigned)((nb + 255) / 256)), 256, 0, h->stream>>>(
                h->rows.ptr.p, h->rows.idx.p, h->rows.val.p, h->user_ids.p, h->item_ids.p, h->table.p, ni, nb, h->out.p);
        } else {
            ease_score_users_kernel<<<dim3((unsigned)((ni + kEaseBlock - 1) / kEaseBlock), (unsigned)nb), kEaseBlock, 0, h->stream>>>(
                h->rows.ptr.p, h->rows.idx.p, h->rows.val.p, h->user_ids.p, h->table.p, ni, h->out.p);
        }
        h->out.download(out + b0 * per_user, (size_t)(nb * per_user), h->stream);
    });
}

int cornac_hip_ease_score_users(cornac_hip_ease_t h, const int32_t *users, int64_t n, double *out) {
    return guarded([&] { ease_score(h, users, nullptr, n, out); });
}

int cornac_hip_ease_score_pairs(cornac_hip_ease_t h, const int32_t *users, const int32_t *items, int64_t n, double *out) {
    return guarded([&] {
        REQUIRE(n == 0 || items != nullptr, "EASE: items is NULL");
        ease_score(h, users, items, n, out);
    });
}

// Building blocks of the row-sharded item table (SURVEY.md §8e regime 2) — included at the end of bpr.hip.
//
// With the item table sharded by row across GPUs a rank cannot run the fused hogwild kernel: the item rows of
// a triplet live on other ranks.  The epoch is cut into micro-batches:
//   bpr_sample_triplets_kernel   draws (u, i, j) with the hogwild sampler (same Philox counters, same
//                                membership test) into device arrays — no table access;
//   [host/RCCL: de-duplicate the item ids, all-to-all the requests, owners gather rows (rows_gather_kernel),
//    all-to-all the rows back into a staging table]
//   bpr_apply_triplets_kernel    the BPR update on the rank's own U rows and the STAGED item rows/biases
//                                (slot indices instead of item ids), fp32 atomics as in hogwild mode;
//   [all-to-all of (staged - fetched) back, owners apply them with rows_scatter_add_kernel]
// cornac_amd/dist.py (RowShardedBprTrainer) drives the sequence on one stream.

namespace chip {

__global__ __launch_bounds__(kBlock) void bpr_sample_triplets_kernel(const HogArgs a, int32_t *__restrict__ out_u,
                                                                     int32_t *__restrict__ out_i,
                                                                     int32_t *__restrict__ out_j, int64_t out_off) {
    unsigned int n_skipped = 0;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < a.n; s += (int64_t)gridDim.x * kBlock) {
        int32_t u, i, j;
        bool in_range;
        const bool valid = hog_sample(a, s, u, i, j, in_range);
        out_u[out_off + s] = valid ? u : -1;
        out_i[out_off + s] = valid ? i : -1;
        out_j[out_off + s] = valid ? j : -1;
        n_skipped += valid ? 0u : 1u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_skipped += __shfl_xor(n_skipped, o, kWave);
    if (lane_id() == 0 && n_skipped) atomicAdd(&a.counters[1], (unsigned long long)n_skipped);
}

// One G-lane group per triplet; U rows of the handle, item rows/biases in the staging table (slot indices).
template <int G>
__global__ __launch_bounds__(kBlock) void bpr_apply_triplets_kernel(const int32_t *__restrict__ tu,
                                                                    const int32_t *__restrict__ si,
                                                                    const int32_t *__restrict__ sj, int64_t n,
                                                                    float *__restrict__ U, float *__restrict__ rows,
                                                                    float *__restrict__ bias, int bias_stride, int k,
                                                                    float lr, float reg, int use_bias,
                                                                    unsigned long long *counters) {
    constexpr int TPW = kWave / G;
    const int lane = lane_id(), grp = lane / G, lg = lane & (G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    unsigned int n_correct = 0;
    for (int64_t base = wave * TPW; base < n; base += n_waves * TPW) {
        const int64_t t = base + grp;
        const bool in = t < n;
        const int32_t u = in ? tu[t] : -1;
        const bool act = u >= 0;
        const int64_t tt = act ? t : 0;
        const int32_t uu = act ? u : 0, a_i = act ? si[tt] : 0, a_j = act ? sj[tt] : 0;
        float *pu = U + (size_t)uu * k, *pi = rows + (size_t)a_i * k, *pj = rows + (size_t)a_j * k;
        float part = 0.f;
        for (int f = lg; f < k; f += G) part += load_f32_fresh(pu + f) * (load_f32_fresh(pi + f) - load_f32_fresh(pj + f));
        const float bi = load_f32_fresh(bias + (size_t)a_i * bias_stride), bj = load_f32_fresh(bias + (size_t)a_j * bias_stride);
        const float score = (bi - bj) + group_sum<G>(part);
        const float z = sigmoid_neg_fast(score);
        if (act) {
            for (int f = lg; f < k; f += G) {
                const float uf = load_f32_fresh(pu + f), vi = load_f32_fresh(pi + f), vj = load_f32_fresh(pj + f);
                atomic_add_f32(pu + f, lr * (z * (vi - vj) - reg * uf));
                atomic_add_f32(pi + f, lr * (z * uf - reg * vi));
                atomic_add_f32(pj + f, lr * (-z * uf - reg * vj));
            }
            if (lg == 0) {
                if (use_bias) {
                    atomic_add_f32(bias + (size_t)a_i * bias_stride, lr * (z - reg * bi));
                    atomic_add_f32(bias + (size_t)a_j * bias_stride, lr * (-z - reg * bj));
                }
                n_correct += z < .5f ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_correct += __shfl_xor(n_correct, o, kWave);
    if (lane == 0 && n_correct) atomicAdd(&counters[0], (unsigned long long)n_correct);
}

// out[r, :] = table[ids[r], :]   (one 16-lane group per row, float4 where the width allows)
__global__ __launch_bounds__(kBlock) void rows_gather_kernel(const float *__restrict__ table,
                                                             const int32_t *__restrict__ ids, int64_t n, int width,
                                                             float *__restrict__ out) {
    const int gl = threadIdx.x & 15;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n; r += ((int64_t)gridDim.x * kBlock) >> 4) {
        const float *src = table + (size_t)ids[r] * width;
        float *dst = out + (size_t)r * width;
        for (int f = gl; f < width; f += 16) dst[f] = src[f];
    }
}

// table[ids[r], :] += delta[r, :]   (ids may repeat across requesters: atomics)
__global__ __launch_bounds__(kBlock) void rows_scatter_add_kernel(float *__restrict__ table,
                                                                  const int32_t *__restrict__ ids, int64_t n,
                                                                  int width, const float *__restrict__ delta) {
    const int gl = threadIdx.x & 15;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n; r += ((int64_t)gridDim.x * kBlock) >> 4) {
        float *dst = table + (size_t)ids[r] * width;
        const float *src = delta + (size_t)r * width;
        for (int f = gl; f < width; f += 16) {
            const float d = src[f];
            if (d != 0.f) atomic_add_f32(dst + f, d);
        }
    }
}

// table[ids[r], :] += (now[r, :] - before[r, :]) * (scale ? scale[r] : 1): the owner's side of a push — `before` is the
// row as the owner sent it, `now` the row as the requester returned it (no delta buffer, no separate subtraction pass)
__global__ __launch_bounds__(kBlock) void rows_scatter_diff_kernel(float *__restrict__ table,
                                                                   const int32_t *__restrict__ ids, int64_t n, int width,
                                                                   const float *__restrict__ now,
                                                                   const float *__restrict__ before,
                                                                   const float *__restrict__ scale) {
    const int gl = threadIdx.x & 15;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n; r += ((int64_t)gridDim.x * kBlock) >> 4) {
        float *dst = table + (size_t)ids[r] * width;
        const float *a = now + (size_t)r * width, *b = before + (size_t)r * width;
        const float sc = scale ? scale[r] : 1.f;
        for (int f = gl; f < width; f += 16) {
            const float d = (__builtin_nontemporal_load(a + f) - __builtin_nontemporal_load(b + f)) * sc;
            if (d != 0.f) atomic_add_f32(dst + f, d);
        }
    }
}

// ---- de-duplication of a micro-batch's item ids without a sort ------------------------------------------------
// owner-major index of item i: g(i) = (i % world) * rows_per_rank + i / world (rank i % world owns it as local row
// i / world), so a scan over g is already bucketed by owner.  mark -> [inclusive scan, on the caller's side] -> slots.
__device__ __forceinline__ int64_t owner_major(int32_t item, int world, int64_t rows_per_rank) {
    return (int64_t)(item % world) * rows_per_rank + item / world;
}

__global__ __launch_bounds__(kBlock) void shard_mark_kernel(const int32_t *__restrict__ ti, const int32_t *__restrict__ tj,
                                                            int64_t n, int world, int64_t rows_per_rank,
                                                            int32_t *__restrict__ mark) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) {
        const int32_t i = ti[t], j = tj[t];
        if (i < 0) continue;  // skipped draw
        mark[owner_major(i, world, rows_per_rank)] = 1;
        mark[owner_major(j, world, rows_per_rank)] = 1;
    }
}

__global__ __launch_bounds__(kBlock) void shard_slots_kernel(const int32_t *__restrict__ ti, const int32_t *__restrict__ tj,
                                                             int64_t n, int world, int64_t rows_per_rank,
                                                             const int32_t *__restrict__ scan,
                                                             int32_t *__restrict__ slot_i, int32_t *__restrict__ slot_j) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) {
        const int32_t i = ti[t], j = tj[t];
        const bool ok = i >= 0;
        slot_i[t] = ok ? scan[owner_major(i, world, rows_per_rank)] - 1 : -1;
        slot_j[t] = ok ? scan[owner_major(j, world, rows_per_rank)] - 1 : -1;
    }
}

// uniq_local[scan[g] - 1] = g % rows_per_rank for every marked g: the request lists, one contiguous run per owner
__global__ __launch_bounds__(kBlock) void shard_uniq_kernel(const int32_t *__restrict__ mark, const int32_t *__restrict__ scan,
                                                            int64_t n_rows, int64_t rows_per_rank,
                                                            int32_t *__restrict__ uniq_local) {
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < n_rows; g += (int64_t)gridDim.x * kBlock)
        if (mark[g]) uniq_local[scan[g] - 1] = (int32_t)(g % rows_per_rank);
}

// ---- regime 1 (replicated item table): the two elementwise passes around the delta all-reduce, fused --------
// bucket = [dV (n*k) | dB (n) | wV (n) | wB (n)],  local = copy of [dV | dB].  The per-row weights w and the reconciled
// update R of a row depend on the rule (S = the row's delta summed over the ranks, after the all-reduce):
//   RULE 0 "sqrt"   w = 1 if this rank touched the row;  R = S / sqrt(max(sum w, 1))
//   RULE 1 "align"  w = |d|^2 of this rank's delta;      R = S * min(1, sum w / |S|^2)
// "align" is the plain sum when the ranks' deltas of a row are orthogonal (independent evidence), their mean when they
// are copies of one step (R ranks that each nearly solved the same hot row: the case in which sum / sqrt(R) overshoots
// and, for MF's unbounded squared-error steps, diverges — tools/emulate_ranks_mf.py); a row one rank touched keeps that
// rank's steps under both rules.  16 lanes per row.
template <int RULE>
__device__ __forceinline__ float delta_group_sum(float v) {  // sum over the 16 lanes of a row group
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    return v;
}

// VEC = 4: k % 4 == 0, a lane moves 16-byte pieces (a 16-lane group covers 256 contiguous bytes per access); VEC = 1 otherwise
template <int VEC>
struct DeltaVec {
    float v[VEC];
    __device__ __forceinline__ static DeltaVec load(const float *p) {
        DeltaVec r;
        if (VEC == 4) {
            const v4f t = *reinterpret_cast<const v4f *>(p);
            r.v[0] = t[0]; r.v[1 % VEC] = t[1]; r.v[2 % VEC] = t[2]; r.v[3 % VEC] = t[3];
        } else {
            r.v[0] = *p;
        }
        return r;
    }
    __device__ __forceinline__ void store(float *p) const {
        if (VEC == 4) {
            v4f t = {v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]};
            *reinterpret_cast<v4f *>(p) = t;
        } else {
            *p = v[0];
        }
    }
};

// The trained table ("flat") is addressed through FlatView: the dense [V (n*k) | B (n)] bucket (pitch k, biases behind
// the rows), or the packed item records of the XCD-strata form (bpr_strata.inc: row r at r * pitch, its bias at
// r * pitch + kp) — the multi-GPU driver's passes then read and write the records the kernel trains on, no unpacking.
// base, bucket and local are always dense.
struct FlatView {
    float *v, *b;        // element (r, f) at v[r * pitch + f], bias r at b[r * bstride]
    int64_t pitch, bstride;
};

template <int RULE, int VEC>
__global__ __launch_bounds__(kBlock) void table_delta_begin_kernel(const FlatView fl_, const float *__restrict__ base,
                                                                   int64_t n, int k, float *__restrict__ bucket,
                                                                   float *__restrict__ local) {
    const int gl = threadIdx.x & 15;
    const int64_t stride = ((int64_t)gridDim.x * kBlock) >> 4;
    const int64_t n_up = (n + stride - 1) / stride * stride;  // whole groups stay in the loop: the shuffles need all 16 lanes
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n_up; r += stride) {
        const bool live = r < n;
        float w = 0.f;
        if (live) {
            for (int f = gl * VEC; f < k; f += 16 * VEC) {
                const int64_t e = r * k + f;
                const DeltaVec<VEC> x = DeltaVec<VEC>::load(fl_.v + r * fl_.pitch + f), bs = DeltaVec<VEC>::load(base + e);
                DeltaVec<VEC> d;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    d.v[q] = x.v[q] - bs.v[q];
                    w += RULE == 0 ? (d.v[q] != 0.f ? 1.f : 0.f) : d.v[q] * d.v[q];
                }
                d.store(bucket + e);
                d.store(local + e);
            }
        }
        w = delta_group_sum<RULE>(w);
        if (live && gl == 0) {
            const int64_t eb = n * k + r;
            const float db = fl_.b[r * fl_.bstride] - base[eb];
            bucket[eb] = db;
            local[eb] = db;
            bucket[n * k + n + r] = RULE == 0 ? (w != 0.f ? 1.f : 0.f) : w;
            bucket[n * k + 2 * n + r] = RULE == 0 ? (db != 0.f ? 1.f : 0.f) : db * db;
        }
    }
}

// the factor S is multiplied with: RULE 0 from the count of touching ranks, RULE 1 from sum |d_r|^2 and |S|^2
template <int RULE>
__device__ __forceinline__ float delta_rule_factor(float w_sum, float s_norm2) {
    if (RULE == 0) return 1.f / sqrtf(fmaxf(w_sum, 1.f));
    return s_norm2 > 0.f ? fminf(1.f, w_sum / s_norm2) : 1.f;
}

template <int RULE, int VEC>
__device__ __forceinline__ float delta_row_norm2(const float *__restrict__ row, int k, int gl, bool live) {
    float s2 = 0.f;
    if (RULE == 1 && live)
        for (int f = gl * VEC; f < k; f += 16 * VEC) {
            const DeltaVec<VEC> t = DeltaVec<VEC>::load(row + f);
#pragma unroll
            for (int q = 0; q < VEC; ++q) s2 += t.v[q] * t.v[q];
        }
    if (RULE == 1) s2 = delta_group_sum<RULE>(s2);
    return s2;
}

// base' = base + R,  flat' = base' + ((flat - base) - local).
// Written this way (not flat += R - local) a row nobody trained since the begin pass ends with flat' == base' BIT FOR
// BIT — (flat - base) reproduces `local` exactly — so the next exchange sees it as untouched; with the other form the
// rounding residue of (flat + (R - local)) - (base + R) marked it as touched and the 1/sqrt(c) rule then discounted
// another rank's genuine update of that row.
template <int RULE, int VEC>
__global__ __launch_bounds__(kBlock) void table_delta_finish_kernel(const FlatView fl_, float *__restrict__ base,
                                                                    const float *__restrict__ bucket,
                                                                    const float *__restrict__ local, int64_t n, int k) {
    const int gl = threadIdx.x & 15;
    const int64_t stride = ((int64_t)gridDim.x * kBlock) >> 4;
    const int64_t n_up = (n + stride - 1) / stride * stride;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n_up; r += stride) {
        const bool live = r < n;
        const float s2 = delta_row_norm2<RULE, VEC>(bucket + (live ? r : 0) * k, k, gl, live);
        if (!live) continue;
        const float cv = delta_rule_factor<RULE>(bucket[n * k + n + r], s2);
        for (int f = gl * VEC; f < k; f += 16 * VEC) {
            const int64_t e = r * k + f;
            float *xp = fl_.v + r * fl_.pitch + f;
            const DeltaVec<VEC> S = DeltaVec<VEC>::load(bucket + e), x = DeltaVec<VEC>::load(xp),
                                b0 = DeltaVec<VEC>::load(base + e), l = DeltaVec<VEC>::load(local + e);
            DeltaVec<VEC> bs, fl;
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                bs.v[q] = b0.v[q] + S.v[q] * cv;
                fl.v[q] = bs.v[q] + ((x.v[q] - b0.v[q]) - l.v[q]);
            }
            fl.store(xp);
            bs.store(base + e);
        }
        if (gl == 0) {
            const int64_t eb = n * k + r;
            float *xb = fl_.b + r * fl_.bstride;
            const float R = bucket[eb] * delta_rule_factor<RULE>(bucket[n * k + 2 * n + r], bucket[eb] * bucket[eb]);
            const float bs = base[eb] + R;
            *xb = bs + ((*xb - base[eb]) - local[eb]);
            base[eb] = bs;
        }
    }
}

// finish of exchange c-1 and begin of exchange c in one pass over the table (they are adjacent in the overlapped
// schedule): apply R_prev, then emit the new delta (which is exactly the work done since begin c-1) and its weights
template <int RULE, int VEC>
__global__ __launch_bounds__(kBlock) void table_delta_step_kernel(const FlatView fl_, float *__restrict__ base,
                                                                  const float *__restrict__ bucket_prev,
                                                                  const float *__restrict__ local_prev, int64_t n, int k,
                                                                  float *__restrict__ bucket, float *__restrict__ local) {
    const int gl = threadIdx.x & 15;
    const int64_t stride = ((int64_t)gridDim.x * kBlock) >> 4;
    const int64_t n_up = (n + stride - 1) / stride * stride;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4; r < n_up; r += stride) {
        const bool live = r < n;
        const float s2 = delta_row_norm2<RULE, VEC>(bucket_prev + (live ? r : 0) * k, k, gl, live);
        float w = 0.f;
        if (live) {
            const float cv = delta_rule_factor<RULE>(bucket_prev[n * k + n + r], s2);
            for (int f = gl * VEC; f < k; f += 16 * VEC) {
                const int64_t e = r * k + f;
                float *xp = fl_.v + r * fl_.pitch + f;
                const DeltaVec<VEC> S = DeltaVec<VEC>::load(bucket_prev + e), x = DeltaVec<VEC>::load(xp),
                                    b0 = DeltaVec<VEC>::load(base + e), l = DeltaVec<VEC>::load(local_prev + e);
                DeltaVec<VEC> bs, fl, d;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    bs.v[q] = b0.v[q] + S.v[q] * cv;
                    fl.v[q] = bs.v[q] + ((x.v[q] - b0.v[q]) - l.v[q]);
                    d.v[q] = fl.v[q] - bs.v[q];
                    w += RULE == 0 ? (d.v[q] != 0.f ? 1.f : 0.f) : d.v[q] * d.v[q];
                }
                fl.store(xp);
                bs.store(base + e);
                d.store(bucket + e);
                d.store(local + e);
            }
        }
        w = delta_group_sum<RULE>(w);
        if (live && gl == 0) {
            const int64_t eb = n * k + r;
            const float R = bucket_prev[eb] * delta_rule_factor<RULE>(bucket_prev[n * k + 2 * n + r], bucket_prev[eb] * bucket_prev[eb]);
            float *xb = fl_.b + r * fl_.bstride;
            const float bs = base[eb] + R, fl = bs + ((*xb - base[eb]) - local_prev[eb]);
            *xb = fl;
            base[eb] = bs;
            const float db = fl - bs;
            bucket[eb] = db;
            local[eb] = db;
            bucket[n * k + n + r] = RULE == 0 ? (w != 0.f ? 1.f : 0.f) : w;
            bucket[n * k + 2 * n + r] = RULE == 0 ? (db != 0.f ? 1.f : 0.f) : db * db;
        }
    }
}

template <int RULE, int VEC>
static void launch_table_delta_rv(int op, unsigned grid, hipStream_t st, const FlatView &fl, float *d_base, const float *d_bucket_prev,
                                  const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local) {
    if (op == 0)
        hipLaunchKernelGGL((table_delta_begin_kernel<RULE, VEC>), dim3(grid), dim3(kBlock), 0, st, fl, (const float *)d_base, n_items, k, d_bucket, d_local);
    else if (op == 1)
        hipLaunchKernelGGL((table_delta_finish_kernel<RULE, VEC>), dim3(grid), dim3(kBlock), 0, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k);
    else
        hipLaunchKernelGGL((table_delta_step_kernel<RULE, VEC>), dim3(grid), dim3(kBlock), 0, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local);
}

// records: the packed item table to use as the trained table instead of d_flat (nullptr: d_flat, dense)
static void launch_table_delta(int op, int rule, hipStream_t st, float *d_flat, float *d_base, const float *d_bucket_prev,
                               const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local,
                               float *records = nullptr, int rec_pitch = 0, int rec_kp = 0) {
    // 8 workgroups per CU, grid-stride: enough bytes in flight for a table of gigabytes, no more launch than a small one needs
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_items * 16 + kBlock - 1) / kBlock, 4096));
    FlatView fl;
    if (records) {
        fl.v = records; fl.pitch = rec_pitch; fl.b = records + rec_kp; fl.bstride = rec_pitch;
    } else {
        fl.v = d_flat; fl.pitch = k; fl.b = d_flat + n_items * (int64_t)k; fl.bstride = 1;
    }
    // 16-byte pieces need every array 16-byte aligned at every row: k % 4 == 0 and aligned bases (torch / hipMalloc
    // buffers are; a sliced view might not be); the records' pitch is a multiple of 32 floats
    auto al16 = [](const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool vec = k % 4 == 0 && al16(fl.v) && al16(d_base) && al16(d_bucket_prev) && al16(d_local_prev) && al16(d_bucket) &&
                     al16(d_local);
    if (rule == 0) {
        if (vec) launch_table_delta_rv<0, 4>(op, grid, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local);
        else launch_table_delta_rv<0, 1>(op, grid, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local);
    } else {
        if (vec) launch_table_delta_rv<1, 4>(op, grid, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local);
        else launch_table_delta_rv<1, 1>(op, grid, st, fl, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local);
    }
}

}  // namespace chip

// ---- the owned kernel in two launches (emit, staged update) around the row exchange -----------------------------
static HogKernel pick_staged_kernel(int k) {
    if (k <= 64) return bpr_hogwild_rowwise_kernel<64, 1, 4, true, true, 2>;
    if (k <= 128) return bpr_hogwild_rowwise_kernel<64, 2, 2, true, true, 2>;
    if (k <= 192) return bpr_hogwild_rowwise_kernel<64, 3, 2, true, true, 2>;
    return bpr_hogwild_rowwise_kernel<64, 4, 1, true, true, 2>;
}

// waves of the grid both launches use (0: this shape has no owned form — k <= 32, k > 256 or too few interactions)
static int64_t staged_waves(cornac_hip_bpr_t h) {
    if (h->k <= 32 || h->k > 256) return 0;
    if (!h->staged_blocks_per_cu) {
        int per_cu = 0;
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pick_staged_kernel(h->k), kBlock, 0));
        // (leaving wave slots free for the fetch / push kernels that run beside this launch on other streams was
        // measured to change nothing: they are slowed by the memory-side atomic queues, not by missing slots)
        h->staged_blocks_per_cu = std::max(1, std::min(per_cu, 8));
    }
    const int64_t W = (int64_t)device_info(h->device).cus * h->staged_blocks_per_cu * kWavesPerBlock;
    return h->nnz >= W * kWave ? W : 0;
}

// tiles of 64 samples every wave runs for the sample range [s_begin, s_begin + n) of an epoch (the kernel's own split)
static void staged_tile_range(cornac_hip_bpr_t h, int64_t s_begin, int64_t n, int64_t *lo, int64_t *hi) {
    *lo = (int64_t)(((unsigned __int128)h->own_tmax * (uint64_t)s_begin) / (uint64_t)h->nnz);
    *hi = s_begin + n >= h->nnz ? h->own_tmax
                                : (int64_t)(((unsigned __int128)h->own_tmax * (uint64_t)(s_begin + n)) / (uint64_t)h->nnz);
}

extern "C" {

int cornac_hip_bpr_sample_triplets(cornac_hip_bpr_t h, int64_t n_draws, int neg_population, int32_t *d_u,
                                   int32_t *d_i, int32_t *d_j) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(h->hog_seeded, "sampling needs cornac_hip_bpr_seed_hogwild first");
        REQUIRE(n_draws >= 0, "n_draws < 0");
        REQUIRE(neg_population == CORNAC_HIP_NEG_UNIFORM || neg_population == CORNAC_HIP_NEG_POPULARITY, "unknown neg_population");
        if (n_draws == 0) return;
        REQUIRE(d_u && d_i && d_j, "output pointers are NULL");
        int64_t left = n_draws, off = 0;
        while (left > 0) {
            const int64_t n = std::min(left, h->nnz - h->hog_offset);
            HogArgs a;
            memset(&a, 0, sizeof a);
            a.user_ids = h->user_ids.p; a.indices = h->indices.p; a.indptr = h->indptr.p;
            a.counters = h->counters.p;
            a.n = n;
            a.s_begin = (uint64_t)h->hog_offset;
            a.seed = h->hog_seed;
            a.epoch = h->hog_epoch;
            a.n_pos = (uint32_t)h->nnz;
            a.neg_items = h->neg_pop_n ? h->neg_pop.p : h->indices.p;
            a.n_neg = neg_population == CORNAC_HIP_NEG_POPULARITY ? (uint32_t)(h->neg_pop_n ? h->neg_pop_n : h->nnz) : (uint32_t)h->n_items;
            a.th_pos = lemire_thresh(a.n_pos);
            a.th_neg = lemire_thresh(a.n_neg);
            a.k = h->k; a.neg_population = neg_population;
            a.nnz = h->nnz;
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 8192));
            hipLaunchKernelGGL(bpr_sample_triplets_kernel, dim3(grid), dim3(kBlock), 0, h->stream, a, d_u, d_i, d_j, off);
            h->hog_offset += n;
            off += n;
            left -= n;
            if (h->hog_offset >= h->nnz) {
                h->hog_offset = 0;
                ++h->hog_epoch;
            }
        }
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_apply_triplets(cornac_hip_bpr_t h, const int32_t *d_u, const int32_t *d_slot_i,
                                  const int32_t *d_slot_j, int64_t n, float *d_rows, float *d_bias, int bias_stride,
                                  float lr, float reg, int use_bias) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0, "n < 0");
        if (n == 0) return;
        REQUIRE(d_u && d_slot_i && d_slot_j && d_rows && d_bias, "NULL device pointer");
        REQUIRE(bias_stride >= 1, "bias_stride must be >= 1");
        const int G = pow2_group(h->k);
        const int tpw = kWave / G;
        const int64_t waves = (n + tpw - 1) / tpw;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + kWavesPerBlock - 1) / kWavesPerBlock, 256 * 16));
#define APPLY(GG)                                                                                                   \
    hipLaunchKernelGGL(bpr_apply_triplets_kernel<GG>, dim3(grid), dim3(kBlock), 0, h->stream, d_u, d_slot_i, d_slot_j, \
                       n, h->U.p, d_rows, d_bias, bias_stride, h->k, lr, reg, use_bias, h->counters.p)
        switch (G) {
            case 4: APPLY(4); break;
            case 8: APPLY(8); break;
            case 16: APPLY(16); break;
            case 32: APPLY(32); break;
            default: APPLY(64); break;
        }
#undef APPLY
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_staged_slots(cornac_hip_bpr_t h, int64_t n_draws, int64_t *n_slots) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n_slots != nullptr && n_draws >= 0, "bad arguments");
        const int64_t W = staged_waves(h);
        *n_slots = 0;
        if (!W) return;
        build_ownership(h, W);
        const int64_t tiles = (int64_t)(((unsigned __int128)h->own_tmax * (uint64_t)n_draws + (uint64_t)h->nnz - 1) / (uint64_t)h->nnz) +
                              n_draws / h->nnz + 2;
        *n_slots = W * tiles * kWave;
    });
}

int cornac_hip_bpr_emit_triplets(cornac_hip_bpr_t h, int64_t n_draws, int neg_population, int32_t *d_u, int32_t *d_i,
                                 int32_t *d_j, int64_t slots_cap, int64_t *n_slots) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(h->hog_seeded, "sampling needs cornac_hip_bpr_seed_hogwild first");
        REQUIRE(n_draws >= 0 && n_slots != nullptr, "bad arguments");
        REQUIRE(neg_population == CORNAC_HIP_NEG_UNIFORM || neg_population == CORNAC_HIP_NEG_POPULARITY, "unknown neg_population");
        *n_slots = 0;
        if (n_draws == 0) return;
        REQUIRE(d_u && d_i && d_j, "output pointers are NULL");
        const int64_t W = staged_waves(h);
        REQUIRE(W > 0, "this shape has no owned kernel (k <= 32, k > 256 or fewer interactions than lanes): use sample_triplets");
        build_ownership(h, W);
        const unsigned grid = (unsigned)(W / kWavesPerBlock);
        int64_t left = n_draws, tile0 = 0;
        while (left > 0) {
            const int64_t n = std::min(left, h->nnz - h->hog_offset);
            HogArgs a;
            memset(&a, 0, sizeof a);
            fill_hog_args(h, a, n, 0.f, 0.f, 0, neg_population, 0);
            a.own_u = h->own_u.p; a.own_i = h->own_i.p; a.wave_ptr = h->wave_ptr.p; a.own_tmax = h->own_tmax;
            int64_t lo, hi;
            staged_tile_range(h, h->hog_offset, n, &lo, &hi);
            a.trip_u = d_u; a.trip_i = d_i; a.trip_j = d_j;
            a.trip_tile0 = tile0;
            a.trip_tiles = hi - lo;
            REQUIRE((tile0 + a.trip_tiles) * W * kWave <= slots_cap, "triplet arrays too small: %lld slots needed",
                    (long long)((tile0 + a.trip_tiles) * W * kWave));
            if (a.trip_tiles > 0)
                hipLaunchKernelGGL((bpr_hogwild_rowwise_kernel<64, 1, 4, true, true, 1>), dim3(grid), dim3(kBlock), 0,
                                   h->stream, a);
            tile0 += a.trip_tiles;
            advance_hog_offset(h, n);
            left -= n;
        }
        HIP_CHECK(hipGetLastError());
        *n_slots = tile0 * W * kWave;
    });
}

int cornac_hip_bpr_apply_staged(cornac_hip_bpr_t h, const int32_t *d_u, const int32_t *d_slot_i, const int32_t *d_slot_j,
                                int64_t n_slots, float *d_rows, float *d_bias, int bias_stride, float lr, float reg,
                                int use_bias) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n_slots >= 0, "n_slots < 0");
        if (n_slots == 0) return;
        REQUIRE(d_u && d_slot_i && d_slot_j && d_rows && d_bias, "NULL device pointer");
        REQUIRE(bias_stride >= 1, "bias_stride must be >= 1");
        const int64_t W = staged_waves(h);
        REQUIRE(W > 0 && h->own_waves == W, "apply_staged follows emit_triplets on the same handle");
        REQUIRE(n_slots % (W * kWave) == 0, "n_slots is not what emit_triplets returned");
        HogArgs a;
        memset(&a, 0, sizeof a);
        fill_hog_args(h, a, 0, lr, reg, use_bias, CORNAC_HIP_NEG_UNIFORM, 0);
        a.V = d_rows;
        a.B = d_bias;
        a.bstride = bias_stride;
        a.trip_u = const_cast<int32_t *>(d_u);
        a.trip_i = const_cast<int32_t *>(d_slot_i);
        a.trip_j = const_cast<int32_t *>(d_slot_j);
        a.trip_tile0 = 0;
        a.trip_tiles = n_slots / (W * kWave);
        h->ktimer.before(h->stream);
        hipLaunchKernelGGL(pick_staged_kernel(h->k), dim3((unsigned)(W / kWavesPerBlock)), dim3(kBlock), 0, h->stream, a);
        h->ktimer.after(h->stream);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_scatter_diff_rows(cornac_hip_bpr_t h, float *d_table, const int32_t *d_ids, int64_t n, int width,
                                     const float *d_now, const float *d_before, const float *d_scale) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0 && width > 0, "bad sizes");
        if (n == 0) return;
        REQUIRE(d_table && d_ids && d_now && d_before, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * 16 + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(rows_scatter_diff_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_table, d_ids, n, width, d_now,
                           d_before, d_scale);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_shard_mark(cornac_hip_bpr_t h, const int32_t *d_i, const int32_t *d_j, int64_t n, int world,
                              int64_t rows_per_rank, int32_t *d_mark) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0 && world >= 1 && rows_per_rank >= 1, "bad sizes");
        if (n == 0) return;
        REQUIRE(d_i && d_j && d_mark, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(shard_mark_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_i, d_j, n, world, rows_per_rank, d_mark);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_shard_slots(cornac_hip_bpr_t h, const int32_t *d_i, const int32_t *d_j, int64_t n, int world,
                               int64_t rows_per_rank, const int32_t *d_scan, int32_t *d_slot_i, int32_t *d_slot_j) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0 && world >= 1 && rows_per_rank >= 1, "bad sizes");
        if (n == 0) return;
        REQUIRE(d_i && d_j && d_scan && d_slot_i && d_slot_j, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(shard_slots_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_i, d_j, n, world, rows_per_rank,
                           d_scan, d_slot_i, d_slot_j);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_shard_uniq(cornac_hip_bpr_t h, const int32_t *d_mark, const int32_t *d_scan, int64_t n_rows,
                              int64_t rows_per_rank, int32_t *d_uniq_local) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n_rows >= 0 && rows_per_rank >= 1, "bad sizes");
        if (n_rows == 0) return;
        REQUIRE(d_mark && d_scan && d_uniq_local, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rows + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(shard_uniq_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_mark, d_scan, n_rows, rows_per_rank,
                           d_uniq_local);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_gather_rows(cornac_hip_bpr_t h, const float *d_table, const int32_t *d_ids, int64_t n, int width,
                               float *d_out) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0 && width > 0, "bad sizes");
        if (n == 0) return;
        REQUIRE(d_table && d_ids && d_out, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * 16 + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(rows_gather_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_table, d_ids, n, width, d_out);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_scatter_add_rows(cornac_hip_bpr_t h, float *d_table, const int32_t *d_ids, int64_t n, int width,
                                    const float *d_delta) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n >= 0 && width > 0, "bad sizes");
        if (n == 0) return;
        REQUIRE(d_table && d_ids && d_delta, "NULL device pointer");
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * 16 + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(rows_scatter_add_kernel, dim3(grid), dim3(kBlock), 0, h->stream, d_table, d_ids, n, width, d_delta);
        HIP_CHECK(hipGetLastError());
    });
}

// The multi-GPU driver's table passes, when the handle trains on packed item records (chunk_records mode, XCD-strata
// form): d_flat is then the driver's dense replica the handle was bound to — stale until cornac_hip_bpr_sync — and the
// pass has to read and write the records instead.  Any other table (or a dense handle): nullptr.
static float *table_delta_records(cornac_hip_bpr_t h, const float *d_flat, int64_t n_items, int k) {
    if (!h->strata_packed) return nullptr;
    // (the records carry the bias too: the flat replica must be [V | B] in one buffer, B right behind V — advisor r4)
    if (d_flat != h->V.p || n_items != h->total_items || k != h->k || h->B.p != h->V.p + (size_t)n_items * (size_t)k) {
        strata_unpack(h);  // (some other table: the dense tables become current first)
        return nullptr;
    }
    return h->VB.p;
}

int cornac_hip_bpr_table_delta_begin(cornac_hip_bpr_t h, const float *d_flat, const float *d_base, int64_t n_items,
                                     int k, float *d_bucket, float *d_local) {
    return guarded([&] {
        bpr_check(h, Records::Keep);  // (the pass works on the packed records when they are what the handle trains on)
        REQUIRE(n_items > 0 && k > 0 && d_flat && d_base && d_bucket && d_local, "bad arguments");
        float *rec = table_delta_records(h, d_flat, n_items, k);
        launch_table_delta(0, 0, h->stream, const_cast<float *>(d_flat), const_cast<float *>(d_base), nullptr, nullptr, n_items,
                           k, d_bucket, d_local, rec, h->vb_pitch, h->vb_kp);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_table_delta_finish(cornac_hip_bpr_t h, float *d_flat, float *d_base, const float *d_bucket,
                                      const float *d_local, int64_t n_items, int k) {
    return guarded([&] {
        bpr_check(h, Records::Keep);  // (the pass works on the packed records when they are what the handle trains on)
        REQUIRE(n_items > 0 && k > 0 && d_flat && d_base && d_bucket && d_local, "bad arguments");
        float *rec = table_delta_records(h, d_flat, n_items, k);
        launch_table_delta(1, 0, h->stream, d_flat, d_base, d_bucket, d_local, n_items, k, nullptr, nullptr, rec, h->vb_pitch,
                           h->vb_kp);
        HIP_CHECK(hipGetLastError());
    });
}

int cornac_hip_bpr_table_delta_step(cornac_hip_bpr_t h, float *d_flat, float *d_base, const float *d_bucket_prev,
                                    const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local) {
    return guarded([&] {
        bpr_check(h, Records::Keep);  // (the pass works on the packed records when they are what the handle trains on)
        REQUIRE(n_items > 0 && k > 0 && d_flat && d_base && d_bucket_prev && d_local_prev && d_bucket && d_local,
                "bad arguments");
        float *rec = table_delta_records(h, d_flat, n_items, k);
        launch_table_delta(2, 0, h->stream, d_flat, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local, rec,
                           h->vb_pitch, h->vb_kp);
        HIP_CHECK(hipGetLastError());
    });
}

// the three passes on the handle's stream with the reconciliation rule as an argument (op: 0 = begin, 1 = finish, 2 = step;
// rule: 0 = sqrt, 1 = align), packed records honoured like the rule-0 entry points above
int cornac_hip_bpr_table_delta(cornac_hip_bpr_t h, int op, int rule, float *d_flat, float *d_base, const float *d_bucket_prev,
                               const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local) {
    return guarded([&] {
        bpr_check(h, Records::Keep);
        REQUIRE(op >= 0 && op <= 2, "op must be 0 (begin), 1 (finish) or 2 (step)");
        REQUIRE(rule == 0 || rule == 1, "rule must be 0 (sqrt) or 1 (align)");
        REQUIRE(n_items > 0 && k > 0 && d_flat && d_base, "bad arguments");
        REQUIRE(op == 0 || (d_bucket_prev && d_local_prev), "finish / step need the previous bucket and local delta");
        REQUIRE(op == 1 || (d_bucket && d_local), "begin / step need the next bucket and local delta");
        float *rec = table_delta_records(h, d_flat, n_items, k);
        launch_table_delta(op, rule, h->stream, d_flat, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local, rec,
                           h->vb_pitch, h->vb_kp);
        HIP_CHECK(hipGetLastError());
    });
}

// the same three passes for a caller without a BPR handle (the MF driver): op & 15: 0 = begin, 1 = finish, 2 = step;
// op >> 4: the reconciliation rule (0 = sqrt, 1 = align)
int cornac_hip_table_delta(int op, int device, void *hip_stream, float *d_flat, float *d_base, const float *d_bucket_prev,
                           const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local) {
    return guarded([&] {
        const int rule = op >> 4;
        op &= 15;
        REQUIRE(op >= 0 && op <= 2, "op must be 0 (begin), 1 (finish) or 2 (step)");
        REQUIRE(rule == 0 || rule == 1, "rule must be 0 (sqrt) or 1 (align)");
        REQUIRE(n_items > 0 && k > 0 && d_flat && d_base, "bad arguments");
        REQUIRE(op == 0 || (d_bucket_prev && d_local_prev), "finish / step need the previous bucket and local delta");
        REQUIRE(op == 1 || (d_bucket && d_local), "begin / step need the next bucket and local delta");
        use_device(device);
        launch_table_delta(op, rule, (hipStream_t)hip_stream, d_flat, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket,
                           d_local);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"

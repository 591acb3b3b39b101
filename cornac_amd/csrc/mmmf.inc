// MMMF (maximum-margin matrix factorisation) on the BPR handle — included at the end of bpr.hip.
//
// Replaces MMMF._fit_sgd (cornac/models/mmmf/recom_mmmf.pyx:103-160): BPR's sampler (two RNGVector engines,
// has_non_zero) under the soft-margin ranking loss.  A triplet whose score is already positive updates nothing
// (:145-147: counted as correct, then `continue`); a violator (score <= 0) takes a step whose size does not depend on
// the score (:150-158), the two biases included — the loop has no use_bias switch.
//
// Same two modes as BPR.  deterministic = the handle's mt19937 streams, level builder and bucketing unchanged
// (bpr_epoch_deterministic), with the hinge kernel below as the kernel of a level; a correct triplet still occupies its
// three rows in the conflict DAG — the schedule exists before any score does — which is exact, only conservative.
// hogwild = Philox + Lemire sampling with the sample numbering of BPR's unowned fused form, then a two-pass wave: the
// score pass costs loads only and retires the skipped and the correct triplets; only the violators reach the update
// pass and its fp32 atomics (DESIGN.md section 1.6).

namespace chip {

// B += lr * (1 - reg * B) as the reference's compiled loop evaluates it (:157-158): the literal is a double, so on float
// tables reg * B is a float product and the rest — the subtraction, the product with lr, the sum — runs in double and is
// rounded once on assignment.  On double tables everything is a double anyway.
template <class T>
__device__ __forceinline__ T mmmf_bias_step(T b, T lr, T reg, double sign) {
    const T rb = reg * b;
    return (T)((double)b + (double)lr * (sign - (double)rb));
}

// One level of the conflict-free schedule under the hinge: the structure of bpr_det_level_kernel (rows read once into
// registers for k <= 4 G, the score summed in index order), the reference's unfused expression trees, no store at all
// for a correct triplet.  T = float or double (`_fit_sgd` is a fused-type function, recom_mmmf.pyx:103-106).
template <int G, class T>
__global__ __launch_bounds__(kBlock) void mmmf_det_level_kernel(const int32_t *__restrict__ su,
                                                                const int32_t *__restrict__ si,
                                                                const int32_t *__restrict__ sj, int64_t off, int cnt,
                                                                T *U, T *V, T *B, int k, T lr, T reg,
                                                                unsigned long long *__restrict__ counters) {
    const int gid = (blockIdx.x * kBlock + threadIdx.x) / G;
    const int lg = threadIdx.x & (G - 1);
    const bool active = gid < cnt;
    const int64_t t = off + (active ? gid : cnt - 1);
    const int32_t u = su[t], i = si[t], j = sj[t];
    T *pu = U + (size_t)u * k, *pi = V + (size_t)i * k, *pj = V + (size_t)j * k;
    const T bi = B[i], bj = B[j];
    T score = bi - bj;  // :141
    constexpr int RMAX = 4;
    T ru[RMAX], ri[RMAX], rj[RMAX];
    const bool in_regs = k <= RMAX * G;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int f = r * G + lg;
        ru[r] = ri[r] = rj[r] = T(0);
        if (in_regs && f < k) {
            ru[r] = pu[f];
            ri[r] = pi[f];
            rj[r] = pj[f];
        }
    }
    auto ordered_add = [&](T p, int lim) { score = ordered_lane_sum_t<G>(score, p, lim); };  // :142-143
    if (in_regs) {
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const int base = r * G;
            if (base < k) ordered_add(base + lg < k ? ru[r] * (ri[r] - rj[r]) : T(0), min(G, k - base));
        }
    } else {
        for (int base = 0; base < k; base += G) {
            const int f = base + lg;
            ordered_add(f < k ? pu[f] * (pi[f] - pj[f]) : T(0), min(G, k - base));
        }
    }
    const bool correct = score > T(0);  // :145 — a score of exactly 0 is a violator
    if (active && !correct) {
        if (in_regs) {
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                const int f = r * G + lg;
                if (f < k) {
                    const T uf = ru[r], vi = ri[r], vj = rj[r];  // uf is `temp` (:151)
                    pu[f] = uf + lr * ((vi - vj) - reg * uf);
                    pi[f] = vi + lr * (uf - reg * vi);
                    pj[f] = vj + lr * (-uf - reg * vj);
                }
            }
        } else {
            for (int f = lg; f < k; f += G) {
                const T uf = pu[f], vi = pi[f], vj = pj[f];
                pu[f] = uf + lr * ((vi - vj) - reg * uf);
                pi[f] = vi + lr * (uf - reg * vi);
                pj[f] = vj + lr * (-uf - reg * vj);
            }
        }
        if (lg == 0) {  // :157-158, no use_bias switch
            B[i] = mmmf_bias_step(bi, lr, reg, 1.0);
            B[j] = mmmf_bias_step(bj, lr, reg, -1.0);
        }
    }
    const unsigned long long m = __ballot(active && lg == 0 && correct);
    if (lane_id() == 0 && m) atomicAdd(&counters[0], (unsigned long long)__popcll(m));
}

template <int G>
__device__ __forceinline__ float mmmf_group_sum(float v) {
    if (G == kWave) return wave_sum_dpp(v);
    return group_sum<G>(v);
}

// Hogwild, k <= G R.  A wave samples a tile of 64 triplets (hog_sample: counter s_begin + local, BPR's Philox key
// layout), drops the skipped ones through LDS, and then works on batches of UNR x (64 / G) triplets, G lanes per
// triplet in the row-wise layout:
//   score pass   the three rows and the two biases of every triplet of the batch are loaded (L1-bypassing, as in
//                bpr_hogwild_rowwise_kernel) and the scores summed; a triplet with score > 0 is counted and retires
//                here, having cost loads only;
//   update pass  the ballot of the violators decides what runs: with no violator in the batch the pass is skipped
//                whole, otherwise only the violators' lane groups are live — a retired group's lanes are off in
//                every atomic instruction, which then touches the violators' lines and no others (for G = 64, one
//                triplet per step, the pass is a wave-uniform branch).  The deltas come from the registers the score
//                was computed from; the two bias deltas are added by the group's first lane.
// A correct triplet issues no atomic, not even of 0.0: no memory write at all.
template <int G, int R, int UNR>
__global__ __launch_bounds__(kBlock) void mmmf_hogwild_kernel(const HogArgs a) {
    __shared__ int32_t stage[kWavesPerBlock][3][kWave];
    constexpr int TPW = kWave / G;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int grp = lane / G, lg = lane & (G - 1);
    const int64_t total_waves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t n_tiles = (a.n + kWave - 1) / kWave;
    bool inb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) inb[r] = lg + G * r < a.k;
    unsigned int n_correct = 0, n_skipped = 0;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wave; tile < n_tiles; tile += total_waves) {
        int32_t su, si, sj;
        bool in_range;
        const bool valid = hog_sample(a, tile * kWave + lane, su, si, sj, in_range);
        const unsigned long long mask = __ballot(valid);
        n_skipped += (in_range && !valid) ? 1u : 0u;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            stage[wave][0][pos] = su;
            stage[wave][1][pos] = si;
            stage[wave][2][pos] = sj;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nvalid = __popcll(mask);
        for (int b = 0; b < nvalid; b += TPW * UNR) {
            float u[UNR][R], vi[UNR][R], vj[UNR][R], bi[UNR], bj[UNR];
            float *pu[UNR], *pi[UNR], *pj[UNR];
            int32_t ti[UNR], tj[UNR];
            bool act[UNR], viol[UNR];
            // ---- score pass: loads only ----
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                const int slot = b + q * TPW + grp;
                act[q] = slot < nvalid;
                const int sl = act[q] ? slot : b;
                const int32_t tu = stage[wave][0][sl];
                ti[q] = stage[wave][1][sl];
                tj[q] = stage[wave][2][sl];
                pu[q] = a.U + (size_t)tu * a.k + lg;
                pi[q] = a.V + (size_t)ti[q] * a.k + lg;
                pj[q] = a.V + (size_t)tj[q] * a.k + lg;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    u[q][r] = inb[r] ? __builtin_nontemporal_load(pu[q] + G * r) : 0.f;
                    vi[q][r] = inb[r] ? __builtin_nontemporal_load(pi[q] + G * r) : 0.f;
                    vj[q][r] = inb[r] ? __builtin_nontemporal_load(pj[q] + G * r) : 0.f;
                }
                bi[q] = __builtin_nontemporal_load(a.B + (size_t)ti[q] * a.bstride);
                bj[q] = __builtin_nontemporal_load(a.B + (size_t)tj[q] * a.bstride);
            }
            unsigned long long any_viol = 0;
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                float part = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) part += u[q][r] * (vi[q][r] - vj[q][r]);
                const float score = (bi[q] - bj[q]) + mmmf_group_sum<G>(part);
                const bool correct = score > 0.f;
                viol[q] = act[q] && !correct;
                n_correct += (act[q] && correct && lg == 0) ? 1u : 0u;
                any_viol |= __ballot(viol[q]);
            }
            if (any_viol == 0) continue;  // the whole batch retired in the score pass
            // ---- update pass: the violators only ----
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                if (!viol[q]) continue;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (inb[r]) {
                        const float uf = u[q][r], xi = vi[q][r], xj = vj[q][r];
                        atomic_add_f32(pu[q] + G * r, a.lr * ((xi - xj) - a.reg * uf));
                        atomic_add_f32(pi[q] + G * r, a.lr * (uf - a.reg * xi));
                        atomic_add_f32(pj[q] + G * r, a.lr * (-uf - a.reg * xj));
                    }
                }
                if (lg == 0) {
                    atomic_add_f32(a.B + (size_t)ti[q] * a.bstride, a.lr * (1.f - a.reg * bi[q]));
                    atomic_add_f32(a.B + (size_t)tj[q] * a.bstride, a.lr * (-1.f - a.reg * bj[q]));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_correct += __shfl_xor(n_correct, o, kWave);
        n_skipped += __shfl_xor(n_skipped, o, kWave);
    }
    if (lane == 0) {
        if (n_correct) atomicAdd(&a.counters[0], (unsigned long long)n_correct);
        if (n_skipped) atomicAdd(&a.counters[1], (unsigned long long)n_skipped);
    }
}

// Hogwild, any k (the dispatcher sends k > 256 here): one triplet per wave step, the 64 lanes stride over the factors.
// The score pass keeps nothing; a violator — a wave-uniform decision — reloads its rows in the update pass.
__global__ __launch_bounds__(kBlock) void mmmf_hogwild_strided_kernel(const HogArgs a) {
    __shared__ int32_t stage[kWavesPerBlock][3][kWave];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t total_waves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t n_tiles = (a.n + kWave - 1) / kWave;
    unsigned int n_correct = 0, n_skipped = 0;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wave; tile < n_tiles; tile += total_waves) {
        int32_t su, si, sj;
        bool in_range;
        const bool valid = hog_sample(a, tile * kWave + lane, su, si, sj, in_range);
        const unsigned long long mask = __ballot(valid);
        n_skipped += (in_range && !valid) ? 1u : 0u;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            stage[wave][0][pos] = su;
            stage[wave][1][pos] = si;
            stage[wave][2][pos] = sj;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nvalid = __popcll(mask);
        for (int b = 0; b < nvalid; ++b) {
            const int32_t tu = stage[wave][0][b], ti = stage[wave][1][b], tj = stage[wave][2][b];
            float *pu = a.U + (size_t)tu * a.k, *pi = a.V + (size_t)ti * a.k, *pj = a.V + (size_t)tj * a.k;
            float part = 0.f;
            for (int f = lane; f < a.k; f += kWave)
                part += __builtin_nontemporal_load(pu + f) *
                        (__builtin_nontemporal_load(pi + f) - __builtin_nontemporal_load(pj + f));
            const float bi = __builtin_nontemporal_load(a.B + (size_t)ti * a.bstride);
            const float bj = __builtin_nontemporal_load(a.B + (size_t)tj * a.bstride);
            const float score = (bi - bj) + wave_sum_dpp(part);
            if (score > 0.f) {
                n_correct += lane == 0 ? 1u : 0u;
                continue;
            }
            for (int f = lane; f < a.k; f += kWave) {
                const float uf = __builtin_nontemporal_load(pu + f), xi = __builtin_nontemporal_load(pi + f),
                            xj = __builtin_nontemporal_load(pj + f);
                atomic_add_f32(pu + f, a.lr * ((xi - xj) - a.reg * uf));
                atomic_add_f32(pi + f, a.lr * (uf - a.reg * xi));
                atomic_add_f32(pj + f, a.lr * (-uf - a.reg * xj));
            }
            if (lane == 0) {
                atomic_add_f32(a.B + (size_t)ti * a.bstride, a.lr * (1.f - a.reg * bi));
                atomic_add_f32(a.B + (size_t)tj * a.bstride, a.lr * (-1.f - a.reg * bj));
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_correct += __shfl_xor(n_correct, o, kWave);
        n_skipped += __shfl_xor(n_skipped, o, kWave);
    }
    if (lane == 0) {
        if (n_correct) atomicAdd(&a.counters[0], (unsigned long long)n_correct);
        if (n_skipped) atomicAdd(&a.counters[1], (unsigned long long)n_skipped);
    }
}

}  // namespace chip

// ---- host ----------------------------------------------------------------------------------------------------
template <int G>
static void launch_mmmf_level(cornac_hip_bpr_t h, const int32_t *ou, const int32_t *oi, const int32_t *oj, int64_t off,
                              int cnt, double lr, double reg) {
    const int groups_per_block = kBlock / G;
    const int grid = (cnt + groups_per_block - 1) / groups_per_block;
    if (h->f64)
        hipLaunchKernelGGL((mmmf_det_level_kernel<G, double>), dim3(grid), dim3(kBlock), 0, h->stream, ou, oi, oj, off, cnt,
                           h->U64.p, h->V64.p, h->B64.p, h->k, lr, reg, h->counters.p);
    else
        hipLaunchKernelGGL((mmmf_det_level_kernel<G, float>), dim3(grid), dim3(kBlock), 0, h->stream, ou, oi, oj, off, cnt,
                           h->U.p, h->V.p, h->B.p, h->k, (float)lr, (float)reg, h->counters.p);
}

// the hinge as the loss of bpr_epoch_deterministic's levels (use_bias is not the loop's to switch)
static void mmmf_det_level_launch(cornac_hip_bpr_t h, int G, const int32_t *ou, const int32_t *oi, const int32_t *oj,
                                  int64_t off, int cnt, double lr, double reg, int) {
    switch (G) {
        case 4: launch_mmmf_level<4>(h, ou, oi, oj, off, cnt, lr, reg); break;
        case 8: launch_mmmf_level<8>(h, ou, oi, oj, off, cnt, lr, reg); break;
        case 16: launch_mmmf_level<16>(h, ou, oi, oj, off, cnt, lr, reg); break;
        case 32: launch_mmmf_level<32>(h, ou, oi, oj, off, cnt, lr, reg); break;
        default: launch_mmmf_level<64>(h, ou, oi, oj, off, cnt, lr, reg); break;
    }
}

// The instantiations: <G, R, UNR> = lanes per triplet, row registers per lane (k <= G R), batches in flight per wave
//   k <= 4    <4, 1, 2>      k <= 64    <64, 1, 4>
//   k <= 8    <8, 1, 2>      k <= 128   <64, 2, 2>
//   k <= 16   <16, 1, 2>     k <= 192   <64, 3, 2>
//   k <= 32   <32, 1, 4>     k <= 256   <64, 4, 1>
//   k > 256   the strided kernel
static HogKernel pick_mmmf_kernel(int k) {
    if (k <= 4) return mmmf_hogwild_kernel<4, 1, 2>;
    if (k <= 8) return mmmf_hogwild_kernel<8, 1, 2>;
    if (k <= 16) return mmmf_hogwild_kernel<16, 1, 2>;
    if (k <= 32) return mmmf_hogwild_kernel<32, 1, 4>;
    if (k <= 64) return mmmf_hogwild_kernel<64, 1, 4>;
    if (k <= 128) return mmmf_hogwild_kernel<64, 2, 2>;
    if (k <= 192) return mmmf_hogwild_kernel<64, 3, 2>;
    if (k <= 256) return mmmf_hogwild_kernel<64, 4, 1>;
    return mmmf_hogwild_strided_kernel;
}

// what every MMMF entry point refuses: the loop has uniform negatives only (recom_mmmf.pyx:129-130 draws j over
// num_items), and the conveyor layout belongs to the LDS-bin form
static void mmmf_check(cornac_hip_bpr_t h) {
    REQUIRE(h->neg_pop_n == 0, "a negative population is set on the handle (cornac_hip_bpr_set_negative_population): "
                               "MMMF draws uniform negatives only, clear it (n = 0)");
    REQUIRE(h->cv_blocks == 0, "the handle is configured for the conveyor (cornac_hip_bpr_conveyor_setup): MMMF has no such form");
}

static void mmmf_hogwild_enqueue(cornac_hip_bpr_t h, int64_t n_samples, float lr, float reg) {
    REQUIRE(h->hog_seeded, "hogwild mode needs cornac_hip_bpr_seed_hogwild first");
    const DeviceInfo &di = device_info(h->device);
    HogKernel kern = pick_mmmf_kernel(h->k);
    if (h->hog_kernel != kern) {
        int per_cu = 0;
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBlock, 0));
        h->hog_kernel = kern;
        h->hog_blocks_per_cu = std::max(1, std::min(per_cu, 8));
    }
    h->Bpad.ensure((size_t)h->total_items * kBiasStride);
    const unsigned bgrid = (unsigned)((h->total_items + kBlock - 1) / kBlock);
    int64_t left = n_samples;
    while (left > 0) {
        const int64_t n = std::min(left, h->nnz - h->hog_offset);
        HogArgs a;
        fill_hog_args(h, a, n, lr, reg, 1, CORNAC_HIP_NEG_UNIFORM, 0);
        a.B = h->Bpad.p;
        a.bstride = kBiasStride;
        hipLaunchKernelGGL(bias_pad_kernel, dim3(bgrid), dim3(kBlock), 0, h->stream, h->B.p, h->Bpad.p, h->total_items);
        const int64_t n_tiles = (n + kWave - 1) / kWave;
        const int64_t want_blocks = (n_tiles + kWavesPerBlock - 1) / kWavesPerBlock;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want_blocks, (int64_t)di.cus * h->hog_blocks_per_cu));
        h->ktimer.before(h->stream);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, h->stream, a);
        HIP_CHECK(hipGetLastError());
        h->ktimer.after(h->stream);
        hipLaunchKernelGGL(bias_unpad_kernel, dim3(bgrid), dim3(kBlock), 0, h->stream, h->Bpad.p, h->B.p, h->total_items);
        advance_hog_offset(h, n);
        left -= n;
    }
}

extern "C" {

int cornac_hip_mmmf_fit_epochs(cornac_hip_bpr_t h, int n_epochs, float lr, float reg, int mode, int64_t *correct,
                               int64_t *skipped) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        REQUIRE(mode == CORNAC_HIP_MODE_DETERMINISTIC || mode == CORNAC_HIP_MODE_HOGWILD, "unknown mode %d", mode);
        REQUIRE(!h->f64, "the handle holds float64 tables: use cornac_hip_mmmf_fit_epochs_f64 (sequential semantics only)");
        mmmf_check(h);
        REQUIRE(mode != CORNAC_HIP_MODE_DETERMINISTIC || h->mt_seeded,
                "deterministic mode needs cornac_hip_bpr_seed_mt19937 first");
        REQUIRE(mode != CORNAC_HIP_MODE_HOGWILD || h->hog_seeded, "hogwild mode needs cornac_hip_bpr_seed_hogwild first");
        if (correct) *correct = 0;
        if (skipped) *skipped = 0;
        for (double &t : h->timing) t = 0;
        Timer total;
        HIP_CHECK(hipMemsetAsync(h->counters.p, 0, 4 * sizeof(unsigned long long), h->stream));
        for (int e = 0; e < n_epochs; ++e) {
            if (mode == CORNAC_HIP_MODE_DETERMINISTIC) {
                bpr_epoch_deterministic(h, lr, reg, 1, CORNAC_HIP_NEG_UNIFORM, mmmf_det_level_launch);
            } else {
                Timer t_k;
                mmmf_hogwild_enqueue(h, h->nnz, lr, reg);
                h->timing[2] += t_k.ms();
            }
        }
        Timer t_sync;
        fetch_counters(h, correct, skipped);
        if (mode == CORNAC_HIP_MODE_HOGWILD) h->timing[2] += t_sync.ms();
        h->timing[3] = total.ms();
    });
}

int cornac_hip_mmmf_fit_epochs_f64(cornac_hip_bpr_t h, int n_epochs, double lr, double reg, int64_t *correct,
                                   int64_t *skipped) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(h->f64, "set float64 tables first (cornac_hip_bpr_set_factors_f64)");
        REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        mmmf_check(h);
        REQUIRE(h->mt_seeded, "deterministic mode needs cornac_hip_bpr_seed_mt19937 first");
        if (correct) *correct = 0;
        if (skipped) *skipped = 0;
        for (double &t : h->timing) t = 0;
        Timer total;
        HIP_CHECK(hipMemsetAsync(h->counters.p, 0, 4 * sizeof(unsigned long long), h->stream));
        for (int e = 0; e < n_epochs; ++e)
            bpr_epoch_deterministic(h, lr, reg, 1, CORNAC_HIP_NEG_UNIFORM, mmmf_det_level_launch);
        fetch_counters(h, correct, skipped);
        h->timing[3] = total.ms();
    });
}

int cornac_hip_mmmf_hogwild_enqueue(cornac_hip_bpr_t h, int64_t n_samples, float lr, float reg) {
    return guarded([&] {
        bpr_check(h, Records::Unpack);
        REQUIRE(n_samples >= 0, "n_samples must be >= 0");
        REQUIRE(!h->f64, "the handle holds float64 tables: use cornac_hip_mmmf_fit_epochs_f64 (sequential semantics only)");
        mmmf_check(h);
        mmmf_hogwild_enqueue(h, n_samples, lr, reg);
    });
}
}

// XCD strata: the throughput form of BPR._fit_sgd (cornac/models/bpr/recom_bpr.pyx:231-267) on gfx950 for catalogues that
// no LDS-bin plan fits — hog_form (bpr.hip) tries the LDS bins first and takes this form by itself from 2^20 items on; the
// multi-GPU driver forces it.
// (textually included by bpr.hip after the handle; device code lives in namespace chip)
//
// The reference's threads update U / V / B rows in place without any synchronisation (racy Hogwild).  On a single
// coherent cache that is plain load-modify-store.  The MI355X has 8 XCDs whose L2s are NOT coherent with each other,
// so the fused kernel (bpr_hogwild_rowwise_kernel) pays for cross-XCD sharing with memory-side fp32 atomics: 10
// 64-byte atomic requests per triplet, the measured wall (DESIGN.md 1.2).  This file removes the sharing instead
// (DSGD strata, Gemulla et al. 2011):
//
//   * items are dealt into 8 partitions, re-dealt every epoch (item_rank = popularity rank; the 8 items of rank group
//     g = rank / 8 go to the 8 partitions rotated by a hash of (g, epoch key): every partition gets one item of every
//     group, so the partitions carry equal popularity mass whatever the skew);
//   * an epoch is 8 launches ("phases"); in phase s the workgroups of XCD x touch ONLY item rows of partition
//     (x + s) % 8: every wave draws its positives from the interactions of its own users whose item is in that
//     partition (per-wave buckets, strata_bucket_kernel, rebuilt on the device once per epoch) and draws the negative
//     uniformly inside the same partition;
//   * hence no item row is touched by two L2s inside a launch, and the kernel boundary (L2 write-back + invalidate)
//     hands a partition to its next XCD: V / B rows are L1-bypassing loads + plain stores served by the owning L2 —
//     the reference's own racy read-modify-write, among the CUs of one XCD only;
//   * the most popular items ("hot": rank < n_hot) would lose most of their updates to that race (dozens of
//     concurrent read-modify-writes of one row); they keep device-scope atomics, which are exact;
//   * U rows stay wave-owned exactly as in the fused kernel (plain, no race at all; shared heavy users atomic).
//
// Which workgroup plays which part is decided at RUN TIME, not by blockIdx (HIP promises nothing about workgroup -> XCD
// placement): a workgroup reads its physical XCD x (HW_REG_XCC_ID), takes the next slot of that XCD from a device
// counter (xcd_claim[x], zeroed before every launch) and becomes virtual workgroup slot * 8 + x: its waves are the
// ownership slices of that virtual workgroup and its partition is (x + phase) % 8 — so the workgroups that touch a
// partition in a launch sit on one XCD by construction and the sample stream stays a pure function of the virtual wave id
// (it has a CPU restatement).  Only if the dispatcher hands an XCD more than grid / 8 workgroups do the surplus ones
// wait until every workgroup has claimed, take the slots the other XCDs left free, and update item rows by atomics for
// that launch (counted: counters[2]) — placement can change speed, never which rows may race.
//
// Sampling contract (bench.py config.sampling): per epoch every wave draws len(bucket) positives i.i.d. from each of
// its 8 buckets (sum = its slice = the fused kernel's count; nnz draws per epoch in total), the negative of a draw is
// uniform over the 1/8 of the items dealt to the positive's partition in that epoch — over epochs every item pair
// meets; draws whose negative is a positive of the user are skipped and counted like recom_bpr.pyx:236-238.

namespace chip {

__device__ __forceinline__ uint32_t xcc_id() {
    return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;  // hwreg(HW_REG_XCC_ID, 0, 4)
}

__global__ void strata_xcd_probe_kernel(uint32_t *__restrict__ out) {
    if (threadIdx.x == 0) out[blockIdx.x] = xcc_id();
}

// rotation of rank group g's 8 items over the 8 partitions in the epoch keyed by `key`
__host__ __device__ __forceinline__ uint32_t strata_rot(uint32_t g, uint32_t key) {
    uint32_t h = g * 0x9E3779B1u + key;
    h ^= h >> 15; h *= 0x85EBCA77u;
    h ^= h >> 13; h *= 0xC2B2AE3Du;
    h ^= h >> 16;
    return h & 7u;
}
__host__ __device__ __forceinline__ uint32_t strata_key(uint64_t seed, uint32_t epoch) {
    uint32_t w[4];
    philox4x32_10(epoch, 0x57A7Au, 0u, 3u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return w[0];
}

constexpr int32_t kHotBit = (int32_t)0x80000000;

struct StrataArgs {
    const int32_t *own_u, *own_i;  // static ownership tables (build_ownership)
    const int64_t *wave_ptr;
    const int32_t *item_rank;      // item -> popularity rank
    int32_t *own_code;             // item_rank[own_i[t]]: static, gathered once (strata_code_kernel) so that the per-epoch
                                   // deal below streams instead of making two random lookups per interaction
    int32_t *rec_u, *rec_i;        // the wave slices re-ordered by partition; rec_i carries kHotBit
    int64_t *sptr;                 // [W * 8 + 1] bucket (w, p) = [sptr[8 w + p], sptr[8 w + p + 1])
    uint32_t key, n_hot;
    int64_t n_waves;
};

// The packed item table of the strata form: record i = [row i (k floats, padded to kp = whole 128-byte lines) | the
// bias's own 128-byte line (bias, 31 zeros)], pitch = kp + 32 floats — row and bias of an item are ONE random location
// (one DRAM page, one translation) instead of two tables' worth.  Measured on the configs[4] slice: the bias accesses
// were 12.7 % of the launch (no-bias ablation 4.75 vs 5.43 ms, profiles/r04_scale_nt_stores.log).
__global__ __launch_bounds__(kBlock) void strata_pack_kernel(const float *__restrict__ V, const float *__restrict__ B,
                                                             int64_t n_items, int k, int kp, int pitch,
                                                             float *__restrict__ VB) {
    const int64_t n = n_items * pitch;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / pitch;
        const int f = (int)(e - i * pitch);
        VB[e] = f < k ? V[i * k + f] : (f == kp ? B[i] : 0.f);
    }
}
__global__ __launch_bounds__(kBlock) void strata_unpack_kernel(const float *__restrict__ VB, int64_t n_items, int k, int kp,
                                                               int pitch, float *__restrict__ V, float *__restrict__ B) {
    const int64_t n = n_items * k;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / k;
        const int f = (int)(e - i * k);
        V[e] = VB[i * pitch + f];
        if (f == 0) B[i] = VB[i * pitch + kp];
    }
}

__global__ __launch_bounds__(kBlock) void strata_code_kernel(const StrataArgs s, int64_t n) {
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock)
        s.own_code[t] = s.item_rank[s.own_i[t]];
}

// one wave per ownership slice: counting sort of the slice's interactions by the partition of their item
__global__ __launch_bounds__(kBlock) void strata_bucket_kernel(const StrataArgs s) {
    const int lane = lane_id();
    const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (w >= s.n_waves) return;
    const int64_t lo = s.wave_ptr[w], hi = s.wave_ptr[w + 1];
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = lo + lane; t < hi; t += kWave) {
        const uint32_t code = (uint32_t)s.own_code[t];
        const uint32_t p = ((code & 7u) + strata_rot(code >> 3, s.key)) & 7u;
#pragma unroll
        for (int q = 0; q < 8; ++q) cnt[q] += (p == (uint32_t)q) ? 1u : 0u;
    }
    int64_t off[8];
    int64_t run = lo;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        uint32_t c = cnt[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
        off[q] = run;
        run += c;
    }
    if (lane < 8) {
        int64_t v = off[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) v = lane == q ? off[q] : v;
        s.sptr[w * 8 + lane] = v;
    }
    if (w == s.n_waves - 1 && lane == 0) s.sptr[s.n_waves * 8] = hi;
    for (int64_t t0 = lo; t0 < hi; t0 += kWave) {
        const int64_t t = t0 + lane;
        const bool in = t < hi;
        int32_t u = 0, i = 0;
        uint32_t p = 8;
        bool hot = false;
        if (in) {
            u = s.own_u[t];
            i = s.own_i[t];
            const uint32_t code = (uint32_t)s.own_code[t];
            p = ((code & 7u) + strata_rot(code >> 3, s.key)) & 7u;
            hot = code < s.n_hot;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned long long m = __ballot(p == (uint32_t)q);
            if (p == (uint32_t)q) {
                const int64_t dst = off[q] + __popcll(m & ((1ull << lane) - 1ull));
                s.rec_u[dst] = u;
                s.rec_i[dst] = hot ? (i | kHotBit) : i;
            }
            off[q] += __popcll(m);
        }
    }
}

// G = 64 lanes per row, R row segments per lane (k <= 64 R), UNR triplets in flight per wave.
// VAR (A/B forms, instantiated in -DCORNAC_PROFILE builds only): bit0 = the user rows are loaded and waited for before
// the item rows are requested (shortens the item rows' load -> store window), bit1 = nt instead of sc1 item-row loads.
// Profile builds also honour a.ablate like the fused kernel; the shipped kernel has no such branches.
#ifdef CORNAC_PROFILE
#define STRATA_ABLATE(bit) ((a.ablate & (bit)) != 0)
#else
#define STRATA_ABLATE(bit) false
#endif
template <int R, int UNR, int VAR = 0>
__global__ __launch_bounds__(kBlock) void bpr_strata_kernel(const HogArgs a) {
    constexpr int G = kWave;
    constexpr int NREF = 2 * UNR;
    __shared__ int32_t stage[kWavesPerBlock][3][kWave];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    // ---- claim a virtual workgroup of this XCD (see the header) ----
    __shared__ uint32_t sh_vblock, sh_misplaced;
    if (threadIdx.x == 0) {
        const uint32_t x = xcc_id(), per = gridDim.x >> 3;  // the host launches a multiple of 8 workgroups
        const uint32_t slot = atomicAdd(&a.xcd_claim[x], 1u);
        uint32_t vb = slot * 8u + x, mis = 0u;
        if (slot >= per) {  // surplus on this XCD: wait for every claim, then take the t-th slot left free elsewhere
            uint32_t t = atomicAdd(&a.xcd_claim[8], 1u);
            for (;;) {
                uint32_t tot = 0;
#pragma unroll
                for (int y = 0; y < 8; ++y) tot += __hip_atomic_load(&a.xcd_claim[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (tot >= gridDim.x) break;
                __builtin_amdgcn_s_sleep(8);
            }
            for (uint32_t y = 0; y < 8u; ++y) {
                const uint32_t c = min(__hip_atomic_load(&a.xcd_claim[y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), per);
                if (t < per - c) {
                    vb = (c + t) * 8u + y;
                    mis = 1u;
                    break;
                }
                t -= per - c;
            }
        }
        sh_vblock = vb;
        sh_misplaced = mis;
    }
    __syncthreads();
    const uint32_t vblock = sh_vblock;
    const bool misplaced = sh_misplaced != 0u;  // workgroup-uniform: item rows fall back to atomics
    const int64_t wave_id = (int64_t)vblock * kWavesPerBlock + wave;
    const uint32_t lxcd = vblock & 7u;
    const uint32_t p = (lxcd + (uint32_t)a.phase) & 7u;
    const int64_t base = a.sptr[wave_id * 8 + p];
    const uint32_t len = (uint32_t)(a.sptr[wave_id * 8 + p + 1] - base);
    const uint32_t th_len = len ? lemire_thresh(len) : 0u;
    // items of partition p: one of every full rank group, plus the partial last group's item if it has one for p
    const uint32_t n_full = (uint32_t)a.n_neg >> 3, rem = (uint32_t)a.n_neg & 7u;
    uint32_t n_p = n_full;
    if (rem && ((p - strata_rot(n_full, a.strata_key)) & 7u) < rem) n_p += 1;
    const uint32_t th_p = n_p ? lemire_thresh(n_p) : 0u;
    const int64_t n_tiles = n_p ? ((int64_t)len + kWave - 1) / kWave : 0;
    unsigned int n_correct = 0, n_skipped = 0;
    if (n_p == 0) n_skipped = lane == 0 ? len : 0;  // (degenerate: no candidate negative in this partition)
    if (misplaced && wave == 0 && lane == 0) atomicAdd(&a.counters[2], 1ull);
    bool inb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) inb[r] = lane + G * r < a.k;
    for (int64_t tile = 0; tile < n_tiles; ++tile) {
        // ---- sample 64 draws, one per lane ----
        const uint32_t local = (uint32_t)(tile * kWave) + lane;
        const bool in_range = local < len;
        uint32_t w[4];
        philox4x32_10(in_range ? local : 0u, (uint32_t)wave_id, a.epoch, 0x10u | p, (uint32_t)a.seed,
                      (uint32_t)(a.seed >> 32), w);
        const uint32_t r_pos = lemire_bounded2(w[0], w[1], len, th_len);
        const uint32_t g = lemire_bounded2(w[2], w[3], n_p, th_p);
        const uint32_t code = g * 8u + ((p - strata_rot(g, a.strata_key)) & 7u);
        const int32_t su = a.rec_u[base + r_pos];
        const int32_t si = a.rec_i[base + r_pos];
        const int32_t j = a.rank_item[code];
        const int32_t u = su < 0 ? ~su : su;
        const bool valid = in_range && (STRATA_ABLATE(1) || !csr_row_contains(a.indices, a.indptr[u], a.indptr[u + 1], j));
        const unsigned long long mask = __ballot(valid);
        n_skipped += (in_range && !valid) ? 1u : 0u;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            stage[wave][0][pos] = su;
            stage[wave][1][pos] = si;
            stage[wave][2][pos] = code < a.n_hot ? (j | kHotBit) : j;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nvalid = __popcll(mask);
        // ---- UNR triplets per step, the whole wave on one row at a time ----
        for (int b = 0; b < nvalid; b += UNR) {
            float u_[UNR][R], v_[NREF][R], bv[NREF];
            float *pu[UNR], *pv[NREF], *pb[NREF];
            int32_t tue[UNR], id[NREF];
            bool act[UNR], hot[NREF];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                act[q] = b + q < nvalid;
                const int sl = act[q] ? b + q : b;
                tue[q] = __builtin_amdgcn_readfirstlane(stage[wave][0][sl]);
                const int32_t ei = __builtin_amdgcn_readfirstlane(stage[wave][1][sl]);
                const int32_t ej = __builtin_amdgcn_readfirstlane(stage[wave][2][sl]);
                const int32_t tu = tue[q] < 0 ? ~tue[q] : tue[q];
                id[2 * q] = ei & ~kHotBit;
                id[2 * q + 1] = ej & ~kHotBit;
                hot[2 * q] = ei < 0 || misplaced;
                hot[2 * q + 1] = ej < 0 || misplaced;
                pu[q] = a.U + (size_t)tu * a.k + lane;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    u_[q][r] = inb[r] && !STRATA_ABLATE(4) ? __builtin_nontemporal_load(pu[q] + G * r) : 0.f;
            }
            if (VAR & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int c = 0; c < NREF; ++c) {
                pv[c] = a.V + (size_t)id[c] * a.vpitch + lane;
                pb[c] = a.B + (size_t)id[c] * a.bstride;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    v_[c][r] = !inb[r] || STRATA_ABLATE(4) ? 0.f
                               : (VAR & 2)                 ? __builtin_nontemporal_load(pv[c] + G * r)
                                                           : load_f32_fresh(pv[c] + G * r);
                bv[c] = STRATA_ABLATE(8) ? 0.f : load_f32_fresh(pb[c]);
            }
            float du[UNR][R], dv[NREF][R], db[NREF];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                float part = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) part += u_[q][r] * (v_[2 * q][r] - v_[2 * q + 1][r]);
                const float score = (bv[2 * q] - bv[2 * q + 1]) + group_sum<G>(part);
                const float z = sigmoid_neg_fast(score);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    du[q][r] = a.lr * (z * (v_[2 * q][r] - v_[2 * q + 1][r]) - a.reg * u_[q][r]);
                    dv[2 * q][r] = a.lr * (z * u_[q][r] - a.reg * v_[2 * q][r]);
                    dv[2 * q + 1][r] = a.lr * (-z * u_[q][r] - a.reg * v_[2 * q + 1][r]);
                }
                db[2 * q] = a.lr * (z - a.reg * bv[2 * q]);
                db[2 * q + 1] = a.lr * (-z - a.reg * bv[2 * q + 1]);
                if (STRATA_ABLATE(16)) {  // lost-update census: column 0 counts a row's positive touches, column 1 its negative ones
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        du[q][r] = 0.f;
                        dv[2 * q][r] = (r == 0 && lane == 0) ? 1.f : 0.f;
                        dv[2 * q + 1][r] = (r == 0 && lane == 1) ? 1.f : 0.f;
                    }
                    db[2 * q] = db[2 * q + 1] = 0.f;
                }
                if (act[q] && lane == 0) n_correct += z < .5f ? 1u : 0u;
            }
            // item rows: hot rows atomically; a cold row is stored once per step by the first triplet naming it,
            // carrying the deltas of every triplet of the step that names it (all of them loaded the same row)
#pragma unroll
            for (int c = 0; c < NREF; ++c) {
                if (!act[c >> 1] || STRATA_ABLATE(2)) continue;
                if (hot[c]) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (inb[r]) atomic_add_f32(pv[c] + G * r, dv[c][r]);
                    if (a.use_bias && lane == 0 && !STRATA_ABLATE(8)) atomic_add_f32(pb[c], db[c]);
                    continue;
                }
                bool lead = true;
#pragma unroll
                for (int c2 = 0; c2 < c; ++c2) lead = lead && !(act[c2 >> 1] && id[c2] == id[c]);
                if (!lead) continue;
                float tot[R], totb = db[c];
#pragma unroll
                for (int r = 0; r < R; ++r) tot[r] = dv[c][r];
#pragma unroll
                for (int c2 = c + 1; c2 < NREF; ++c2) {
                    if (act[c2 >> 1] && id[c2] == id[c]) {
#pragma unroll
                        for (int r = 0; r < R; ++r) tot[r] += dv[c2][r];
                        totb += db[c2];
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (inb[r]) {
                        if (STRATA_ABLATE(128)) __builtin_nontemporal_store(v_[c][r] + tot[r], pv[c] + G * r);  // (experiment)
                        else pv[c][G * r] = v_[c][r] + tot[r];
                    }
                // the bias has a 128-byte line of the padded table to itself: the whole line is stored (a 4-byte store
                // leaves a partial line that the memory side has to read-modify-write: measured 18 % of the launch)
                if (a.use_bias && !STRATA_ABLATE(8)) {
                    if (a.bstride >= kBiasStride && !STRATA_ABLATE(32)) {
                        if (lane < kBiasStride) pb[c][lane] = lane == 0 ? bv[c] + totb : 0.f;
                    } else if (lane == 0) {
                        *pb[c] = bv[c] + totb;
                    }
                }
            }
            // user rows: exclusive to this wave (plain store of u_old + the deltas of every triplet of the step with the
            // same user); shared heavy users atomically
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                if (!act[q] || STRATA_ABLATE(2)) continue;
                if (tue[q] < 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (inb[r]) atomic_add_f32(pu[q] + G * r, du[q][r]);
                    continue;
                }
                float tot[R];
#pragma unroll
                for (int r = 0; r < R; ++r) tot[r] = du[q][r];
#pragma unroll
                for (int q2 = 0; q2 < UNR; ++q2) {
                    if (q2 != q && act[q2] && tue[q2] == tue[q]) {
#pragma unroll
                        for (int r = 0; r < R; ++r) tot[r] += du[q2][r];
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (inb[r]) {
                        if (STRATA_ABLATE(64)) __builtin_nontemporal_store(u_[q][r] + tot[r], pu[q] + G * r);  // (experiment)
                        else pu[q][G * r] = u_[q][r] + tot[r];
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

}  // namespace chip

// LDS-resident item bins: the default throughput form of BPR._fit_sgd (cornac/models/bpr/recom_bpr.pyx:231-267) on
// gfx950 for item tables that fit the chip's LDS in a few rounds.  (textually included by bpr.hip)
//
// What bounds the fused kernel (bpr_hogwild_rowwise_kernel) is the 10 memory-side fp32 atomic requests a triplet needs
// because any CU may update any item row (DESIGN.md 1.2); what breaks plain read-modify-write instead (the XCD-strata
// form, bpr_strata.inc) is that an item table of a few 10^4 rows is updated every few microseconds per row, so a third
// of the updates collide inside a load -> store window (measured, tools/strata_census.py).  An item row has to live
// where a read-modify-write is cheap AND exclusive: in the LDS of ONE CU.
//
//   * per epoch the items are dealt into B bins (B = a multiple of the CU count).  The deal (ldsbin_deal_item below):
//     the popularity ranks are cut into strata of ~strata_groups * B consecutive ranks (default 16 B); inside a stratum
//     the ranks are permuted by an epoch-keyed bijection (ldsbin_perm), the permuted sequence is cut into groups of B,
//     and group g goes to the B bins rotated by a hash of (g, epoch key).  Every bin therefore holds the same number of
//     items of every popularity stratum (~n_items / B rows in all: 105 rows = 27 KB at the ML-20M shape), and ANY two
//     items share a bin in an epoch with probability 1 / B (different strata) or (1 - 1 / strata_groups) / B (same
//     stratum: they must fall into different groups) — no pair is excluded.  (Round 3 cut the groups from the static
//     rank order: two items of one rank group of B could never meet.  tests/test_ldsbin_deal_cpu.py counts the pairs.)
//   * one 16-wave workgroup per bin keeps the bin's rows and biases in LDS for the whole epoch: it draws its
//     positives i.i.d. from the interactions of its own items (the CSC segments of its items: sum of their degrees
//     draws per epoch, nnz in total), draws the negative uniformly among the OTHER items of the same bin, tests it against
//     the user's row (has_non_zero, recom_bpr.pyx:46-51: a bitmap probe, or the CSR binary search when the bitmap
//     would not fit), and applies the item-side updates as plain LDS read-modify-writes under a per-row lock: exact,
//     no update lost, no memory-side atomic;
//   * user rows can be touched by any bin: fp32 atomics (2 line requests per triplet at k = 64 instead of 6);
//   * the few items whose degree exceeds hot_x1000 / 1000 of a bin's share ("hot") would serialise their bin: their
//     rows stay in global memory under device-scope atomics and their interactions (a list shuffled once at build time)
//     are dealt to the bins in contiguous runs whose lengths level the bins' work: a permuted stratum gives a bin a
//     random sample of its ranks, so the bins' own ("cold") masses differ by ~10 %, and one workgroup per CU means the
//     heaviest bin sets the epoch's time.  ldsbin_level_kernel fills the light bins up with hot interactions (a hot draw
//     priced at hot_cost_x16 / 16 cold draws) — every interaction is still drawn by exactly one bin.
//
// Sampling contract (bench.py config.sampling): every interaction is drawn with the reference's probability 1 / nnz
// per draw, nnz draws per epoch; the negative of a draw is uniform over the ~n_items / B items that share the
// positive's bin in that epoch; bins are re-dealt every epoch and every (positive, negative) pair of items can meet
// (see the deal above; 256 bins at the ML-20M shape train like the global draw — tools/sim_binned_negatives.py,
// DESIGN.md 1.2).  No launch-order or placement assumption: a bin is private to its workgroup, the sample stream is a
// pure function of (seed, epoch, bin, draw).

//
// Resident exchange (EXCH instantiations; multi-GPU regime 1, DESIGN.md 5): the replicated item table is reconciled across
// ranks n_ex times per epoch WITHOUT cutting the epoch into chunk launches.  The bin's workgroup itself publishes the
// deltas of its rows at the exchange points (the rows live in its LDS: nobody else could) and applies the summed deltas
// of the other ranks once they have landed — it never waits for either:
//   * boundary e of a bin sits at tile (e + 1) * (n_tiles / n_ex); its duty is cut into P <= 16 parts that ride on the
//     P tiles from there on: the wave that claims such a tile first does the part's rows (slots s = part mod P, the hot
//     rows h = bin mod n_bins with part 0) and then processes its tile as usual;
//   * a row's duty: (1) for every exchange that has LANDED (flag set by the communication stream after the all-reduce)
//     and that this part has not applied yet, row += c and base += c with c = rule(S) - keep, S the all-reduced delta,
//     keep this rank's own contribution; (2) publish d = row - base into bucket e (write-through stores) and keep e,
//     base = row.  Under the row's LDS lock, so a step of another wave is either in d or in the next delta, never lost;
//   * the part's wave drains its stores (vmcnt 0) and counts the part done in LDS; the last part of the boundary bumps
//     the exchange's arrival counter (system scope).  The communication stream waits for n_bins arrivals
//     (stream_wait_counter_kernel), all-reduces the bucket in place and sets the landed flag;
//   * at the end of the launch all 16 waves do the last boundary's duty; every row records how many exchanges it has
//     applied, and ldsbin_exchange_flush_kernel (after the last all-reduce) applies the rest.
// Invariant: row - base = this rank's steps since the row's last publication; a row nobody stepped stays equal to its
// base bit for bit (row and base receive the same c), so it publishes an exact zero and counts as untouched.

namespace chip {

constexpr int kLbBlock = 1024;
constexpr int kLbWaves = kLbBlock / kWave;
constexpr int32_t kLbHot = (int32_t)0x80000000;
constexpr int kLbMaxExchanges = 32;
constexpr int kLbMaxRanges = 8;   // bin ranges (= conveyor blocks, one per ring) a conveyor launch covers

// buffers of the resident exchange; all dense, laid out like ItemTableReplica's (cornac_amd/dist.py)
struct LdsBinExchange {
    float *base;                  // [nt k + nt]
    float *bucket;                // exchange e at bucket + e * bucket_stride: [dV (nt k) | dB (nt) | wV (nt) | wB (nt)]
    float *keep;                  // exchange e at keep + e * keep_stride: [dV | dB] as published (the all-reduce is in place)
    unsigned int *arrive;         // [n_ex] workgroups that have published exchange e
    const unsigned int *landed;   // [n_ex] != 0: bucket e holds the sum over the ranks
    unsigned int *applied;        // [n_items] out: exchanges [0, applied[i]) have been applied to row i by its owner
    long long bucket_stride, keep_stride;
    long long nt;                 // rows of the replicated table
    int n_ex, rule;               // rule: 0 "sqrt", 1 "align" (sharded.inc)
};

struct LdsBinArgs {
    const int32_t *cptr, *cusers;     // CSC of the interaction matrix: users of item i at [cptr[i], cptr[i+1])
    const int32_t *rank_item;         // popularity rank -> item
    const int32_t *hot_u, *hot_i;     // interactions of the hot items (rank < n_hot), shuffled once at build time
    const uint32_t *hot_off;          // [n_bins + 1]: bin b draws the hot interactions [hot_off[b], hot_off[b + 1])
    const int32_t *indptr, *indices;  // CSR (membership test without a bitmap)
    const uint32_t *bitmap;           // [n_users][bm_words] or NULL
    float *U, *V, *B;
    unsigned long long *counters;
    uint64_t seed;
    uint32_t epoch, key;
    int32_t n_items, n_bins, n_hot, n_hot_inter, bm_words, cap;  // cap = LDS rows per bin = ceil(n_items / n_bins)
    int32_t n_strata;                 // popularity strata of the deal (ldsbin_deal_item)
    unsigned long long *wg_clock;     // profile build: [n_bins][2] wall clock at entry / exit of the bin's workgroup, or NULL
    int k, use_bias;
    float lr, reg;
    int ablate;
    // WBPR (recom_wbpr.pyx:131-139: the negative is the item of a uniformly drawn interaction, i.e. popularity-weighted):
    // the negative of a draw is the item of a second interaction drawn from the bin's own draw space — a cold
    // interaction names a slot of the bin, a hot one its (global) item — with the positive slot's interactions left out
    int neg_pop;
    // a launch covers the fraction [s_begin, s_begin + n) / nnz of EVERY bin's draws of the epoch (whole epoch: 0, nnz)
    uint64_t s_begin, n, nnz;
    LdsBinExchange ex;                // EXCH instantiations only (whole epochs)
    // Conveyor (multi-GPU regime 2, cornac_amd/dist.py BinConveyorBprTrainer; DESIGN.md 5): conv_bpb != 0 — the launch's
    // workgroups cover conv ranges of conv_bpb consecutive bins (a conveyor BLOCK = the bins [B conv_bpb, (B + 1) conv_bpb)
    // of the epoch's deal, so a block's items change with the epoch key like any bin's); range r starts at bin conv_first[r]
    // and the rows of its bins are NOT in the item-ordered table V / B but in the block's buffer conv_rows[r], in (bin,
    // slot) order: row (b - conv_first[r]) cap + s at conv_rows[r] + that k, its bias at conv_rows[r] + conv_bpb cap k +
    // that.  No hot items in this layout (n_hot = 0, hot_off all zero).
    int32_t conv_bpb;
    int32_t conv_first[kLbMaxRanges];
    float *conv_rows[kLbMaxRanges];
    // Pre-sampled launches (ldsbin_presample_kernel + the PRE instantiations): the tiles of bin b are the records
    // pre_base[b] + tile of the pool — pre_rec: [pool][3][64] (user, positive reference, negative reference of the tile's VALID
    // triplets, compacted), pre_cnt: [pool] how many.  pre_waves: waves of the training workgroup (it fixes the tile width).
    int32_t *pre_rec;
    uint32_t *pre_cnt;
    const uint32_t *pre_base;
    uint32_t pre_waves;
};

__host__ __device__ __forceinline__ uint32_t ldsbin_rot(uint32_t g, uint32_t key, uint32_t n_bins) {
    uint32_t h = g * 0x9E3779B1u + key;
    h ^= h >> 15; h *= 0x85EBCA77u;
    h ^= h >> 13; h *= 0xC2B2AE3Du;
    h ^= h >> 16;
    return h % n_bins;
}

// the mixer and the keyed bijection of [0, n) live in rng.h (mix32, feistel_perm)
__host__ __device__ __forceinline__ uint32_t ldsbin_mix(uint32_t h) { return mix32(h); }
__host__ __device__ __forceinline__ uint32_t ldsbin_perm(uint32_t x, uint32_t n, uint32_t key) { return feistel_perm(x, n, key); }

// The deal.  n_groups = ceil(n_items / n_bins) groups of n_bins positions; stratum s of n_strata covers the groups
// [s n_groups / n_strata, (s + 1) n_groups / n_strata) and the ranks of their positions (the last one ends at n_items).
// Position p = g n_bins + o holds the item of rank base_s + perm_s(p - base_s) and belongs to bin (o + rot(g)) mod n_bins.
// Returns the popularity rank at position p (p < n_items).
__host__ __device__ inline uint32_t ldsbin_deal_rank(uint32_t p, uint32_t key, uint32_t n_bins, uint32_t n_items,
                                                     uint32_t n_groups, uint32_t n_strata) {
    const uint32_t g = p / n_bins;
    uint32_t s = (uint32_t)(((uint64_t)g * n_strata) / n_groups);
    if ((uint32_t)(((uint64_t)(s + 1u) * n_groups) / n_strata) <= g) ++s;
    const uint32_t g_lo = (uint32_t)(((uint64_t)s * n_groups) / n_strata);
    const uint32_t g_hi = (uint32_t)(((uint64_t)(s + 1u) * n_groups) / n_strata);
    const uint32_t base = g_lo * n_bins;
    const uint64_t end = (uint64_t)g_hi * n_bins;
    const uint32_t size = (uint32_t)(end < (uint64_t)n_items ? end : (uint64_t)n_items) - base;
    return base + ldsbin_perm(p - base, size, key ^ ldsbin_mix(s * 0x27D4EB2Fu + 0x165667B1u));
}

#ifdef CORNAC_PROFILE
#define LB_ABLATE(bit) ((a.ablate & (bit)) != 0)
#else
#define LB_ABLATE(bit) false
#endif

// ---- resident exchange: one row's duty ---------------------------------------------------------------------------
// the factor the summed delta S of a row is multiplied with (delta_rule_factor of sharded.inc, rule at run time)
__host__ __device__ __forceinline__ float ex_rule_factor(int rule, float w_sum, float s_norm2) {
    if (rule == 0) return 1.f / sqrtf(fmaxf(w_sum, 1.f));
    return s_norm2 > 0.f ? fminf(1.f, w_sum / s_norm2) : 1.f;
}
// write-through store that also a peer reading the bucket over xGMI sees once the wave's vmcnt has drained
__device__ __forceinline__ void store_f32_system(float *p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Acquire an LDS row lock for the whole wave (lane 0 spins).  A holder never waits for anything, so the spin only ends
// by acquisition; the bound turns a would-be hang (a bug) into a counted, visible event (*timeouts = counters[3],
// cornac_hip_bpr_ldsbin_stats) — the wave then goes on WITHOUT the lock and must not release it (returns false).
__device__ __forceinline__ bool lds_row_lock(int *lock, int lane, unsigned long long *timeouts) {
    int owned = 1;
    if (lane == 0) {
        int spins = 0;
        while (atomicCAS(lock, 0, 1) != 0) {
            if (++spins > (1 << 22)) {
                atomicAdd(timeouts, 1ull);
                owned = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    owned = __builtin_amdgcn_readfirstlane(owned);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return owned != 0;
}
__device__ __forceinline__ void lds_row_unlock(int *lock, int lane, bool owned) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (owned && lane == 0) __hip_atomic_store(lock, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The whole wave on row `it` (lane f holds the factors f, f + 64, ...): applies the exchanges [e_lo, e_hi) (landed, not
// yet applied to this row) and publishes the row's delta of exchange e_pub.  lds_row / lds_bias: the row's home in the
// bin's LDS (lock: its row lock while other waves still train; nullptr once they have stopped), or nullptr for a hot
// row, whose home is the global table under device-scope atomics.
template <int R>
__device__ __forceinline__ void ex_row_duty(const LdsBinExchange &x, float *__restrict__ gV, float *__restrict__ gB, int k,
                                            int32_t it, float *lds_row, float *lds_bias, int *lock, int e_lo, int e_hi,
                                            int e_pub, int lane, const bool (&inb)[R], unsigned long long *timeouts) {
    constexpr int G = kWave;
    const size_t nk = (size_t)x.nt * (size_t)k, ro = (size_t)it * (size_t)k + (size_t)lane;
    float c[R], cb = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = 0.f;
    for (int e = e_lo; e < e_hi; ++e) {  // c = sum over the landed exchanges of rule(S) - keep   (loads, no lock held)
        const float *S = x.bucket + (size_t)e * (size_t)x.bucket_stride;
        const float *K = x.keep + (size_t)e * (size_t)x.keep_stride;
        float s[R], n2 = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            s[r] = inb[r] ? load_f32_fresh(S + ro + G * r) : 0.f;
            n2 += s[r] * s[r];
        }
        const float sb = load_f32_fresh(S + nk + it);
        const float wv = load_f32_fresh(S + nk + (size_t)x.nt + it), wb = load_f32_fresh(S + nk + 2 * (size_t)x.nt + it);
        if (x.rule != 0) n2 = group_sum<G>(n2);
        const float fv = ex_rule_factor(x.rule, wv, n2), fb = ex_rule_factor(x.rule, wb, sb * sb);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (inb[r]) c[r] += s[r] * fv - K[ro + G * r];
        cb += sb * fb - K[nk + it];
    }
    float bs[R], row[R], rb;
#pragma unroll
    for (int r = 0; r < R; ++r) bs[r] = inb[r] ? x.base[ro + G * r] : 0.f;
    const float bb = x.base[nk + it];
    const bool any = e_hi > e_lo;
    if (lds_row) {
        const bool owned = lock ? lds_row_lock(lock, lane, timeouts) : false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            row[r] = lds_row[lane + G * r] + c[r];
            if (any) lds_row[lane + G * r] = row[r];
        }
        rb = *lds_bias + cb;
        if (any && lane == 0) *lds_bias = rb;
        if (lock) lds_row_unlock(lock, lane, owned);
    } else {
        // hot row: other workgroups add to it at any time; the returning atomic gives ONE value per element that both the
        // delta and the new base are taken from, so a concurrent step is in this delta or in the next one
#pragma unroll
        for (int r = 0; r < R; ++r)
            row[r] = !inb[r] ? 0.f
                     : any   ? __hip_atomic_fetch_add(gV + ro + G * r, c[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + c[r]
                             : load_f32_fresh(gV + ro + G * r);
        float t = 0.f;
        if (lane == 0) t = any ? __hip_atomic_fetch_add(gB + it, cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + cb : load_f32_fresh(gB + it);
        rb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t)));
    }
    // publish: d = row - (base + c)  (row and base took the same c: an unstepped row gives an exact zero), base = row
    float *Bk = x.bucket + (size_t)e_pub * (size_t)x.bucket_stride;
    float *Kp = x.keep + (size_t)e_pub * (size_t)x.keep_stride;
    float w = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!inb[r]) continue;
        const float d = row[r] - (bs[r] + c[r]);
        w += x.rule == 0 ? (d != 0.f ? 1.f : 0.f) : d * d;
        store_f32_system(Bk + ro + G * r, d);
        Kp[ro + G * r] = d;
        x.base[ro + G * r] = row[r];
    }
    w = group_sum<G>(w);
    if (lane == 0) {
        const float db = rb - (bb + cb);
        store_f32_system(Bk + nk + it, db);
        Kp[nk + it] = db;
        x.base[nk + it] = rb;
        store_f32_system(Bk + nk + (size_t)x.nt + it, x.rule == 0 ? (w != 0.f ? 1.f : 0.f) : w);
        store_f32_system(Bk + nk + 2 * (size_t)x.nt + it, x.rule == 0 ? (db != 0.f ? 1.f : 0.f) : db * db);
    }
}

// NB cold rows of one part at a time (the in-launch duty): what ex_row_duty does for one row, with the global loads of
// all NB rows issued before the first of them is used — a duty is a chain of dependent memory round trips (the sums,
// the bases), ~3 us per row one after the other; in groups of NB the trips overlap.  its[q] < 0: no row.
template <int R, int NB>
__device__ __forceinline__ void ex_rows_duty(const LdsBinExchange &x, int k, const int32_t (&its)[NB], float *const (&lds_row)[NB],
                                             float *const (&lds_bias)[NB], int *const (&lock)[NB], int e_lo, int e_hi, int e_pub,
                                             int lane, const bool (&inb)[R], unsigned long long *timeouts) {
    constexpr int G = kWave;
    const size_t nk = (size_t)x.nt * (size_t)k;
    size_t ro[NB];
    bool on[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        on[q] = its[q] >= 0;
        ro[q] = (size_t)(on[q] ? its[q] : 0) * (size_t)k + (size_t)lane;
    }
    float c[NB][R], cb[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        cb[q] = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) c[q][r] = 0.f;
    }
    for (int e = e_lo; e < e_hi; ++e) {
        const float *S = x.bucket + (size_t)e * (size_t)x.bucket_stride;
        const float *K = x.keep + (size_t)e * (size_t)x.keep_stride;
        float sv[NB][R], kv[NB][R], sb[NB], wv[NB], wb[NB], kb[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) {  // every load of the group first
            const size_t it = on[q] ? (size_t)its[q] : 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                sv[q][r] = (on[q] && inb[r]) ? load_f32_fresh(S + ro[q] + G * r) : 0.f;
                kv[q][r] = (on[q] && inb[r]) ? K[ro[q] + G * r] : 0.f;
            }
            sb[q] = load_f32_fresh(S + nk + it);
            wv[q] = load_f32_fresh(S + nk + (size_t)x.nt + it);
            wb[q] = load_f32_fresh(S + nk + 2 * (size_t)x.nt + it);
            kb[q] = K[nk + it];
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            float n2 = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) n2 += sv[q][r] * sv[q][r];
            if (x.rule != 0) n2 = group_sum<G>(n2);
            const float fv = ex_rule_factor(x.rule, wv[q], n2), fb = ex_rule_factor(x.rule, wb[q], sb[q] * sb[q]);
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (inb[r]) c[q][r] += sv[q][r] * fv - kv[q][r];
            cb[q] += sb[q] * fb - kb[q];
        }
    }
    float bs[NB][R], bb[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
#pragma unroll
        for (int r = 0; r < R; ++r) bs[q][r] = (on[q] && inb[r]) ? x.base[ro[q] + G * r] : 0.f;
        bb[q] = x.base[nk + (on[q] ? (size_t)its[q] : 0)];
    }
    const bool any = e_hi > e_lo;
    float row[NB][R], rb[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        if (!on[q]) continue;  // (wave-uniform)
        const bool owned = lds_row_lock(lock[q], lane, timeouts);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            row[q][r] = lds_row[q][lane + G * r] + c[q][r];
            if (any) lds_row[q][lane + G * r] = row[q][r];
        }
        rb[q] = *lds_bias[q] + cb[q];
        if (any && lane == 0) *lds_bias[q] = rb[q];
        lds_row_unlock(lock[q], lane, owned);
    }
    float *Bk = x.bucket + (size_t)e_pub * (size_t)x.bucket_stride;
    float *Kp = x.keep + (size_t)e_pub * (size_t)x.keep_stride;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        if (!on[q]) continue;
        const size_t it = (size_t)its[q];
        float w = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!inb[r]) continue;
            const float d = row[q][r] - (bs[q][r] + c[q][r]);
            w += x.rule == 0 ? (d != 0.f ? 1.f : 0.f) : d * d;
            store_f32_system(Bk + ro[q] + G * r, d);
            Kp[ro[q] + G * r] = d;
            x.base[ro[q] + G * r] = row[q][r];
        }
        w = group_sum<G>(w);
        if (lane == 0) {
            const float db = rb[q] - (bb[q] + cb[q]);
            store_f32_system(Bk + nk + it, db);
            Kp[nk + it] = db;
            x.base[nk + it] = rb[q];
            store_f32_system(Bk + nk + (size_t)x.nt + it, x.rule == 0 ? (w != 0.f ? 1.f : 0.f) : w);
            store_f32_system(Bk + nk + 2 * (size_t)x.nt + it, x.rule == 0 ? (db != 0.f ? 1.f : 0.f) : db * db);
        }
    }
}

// dynamic LDS: rows[cap][KP] | bias[cap] | item[cap] | cp[cap] | cum[cap + 1] | lock[cap] | stage[16][3][64]
// POP: popularity-weighted negatives (WBPR, a.neg_pop) — a template parameter so that the BPR instantiation carries
// nothing of it
// PF: how many steps ahead the user rows are requested (1: resident bins — 16 waves per CU at the atomic-request ceiling;
// 2: passing bins, whose 8-wave workgroups are bound by the latency chain of a wave's own steps)
// ---- a bin's slot tables and its draws: shared by the training kernel and by ldsbin_presample_kernel -------------------
struct LdsBinCtx {
    const int32_t *item, *cp;    // LDS: slot -> item (| kLbHot), first CSC position of its users
    const uint32_t *cum;         // LDS: exclusive scan of the slots' degrees ([n_slots + 1])
    uint32_t b, n_slots, cold_mass, hot_lo, n_draws, th_draw, th_slot, th_slot1;
};

struct LdsBinDraw {
    int32_t u, ei, ej, j;
    bool in_range;
};

// slot g of bin b holds the item of group g dealt to it (the last group may have none); all threads of the workgroup call
// this (two barriers).  lock may be NULL.  Leaves n_slots / cold mass in the shared scalars.
__device__ __forceinline__ void ldsbin_build_tables(const LdsBinArgs &a, uint32_t b, uint32_t nb, uint32_t n_groups, int32_t *item,
                                                    int32_t *cp, uint32_t *cum, int *lock, uint32_t *sh_nslots,
                                                    uint32_t *sh_cold_mass, uint32_t *sh_next_tile) {
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t g = threadIdx.x; g < n_groups; g += blockDim.x) {
        const uint32_t pos = g * nb + (b + nb - ldsbin_rot(g, a.key, nb)) % nb;
        int32_t it = -1, c0 = 0;
        uint32_t d = 0;
        if (pos < (uint32_t)a.n_items) {
            const uint32_t code = ldsbin_deal_rank(pos, a.key, nb, (uint32_t)a.n_items, n_groups, (uint32_t)a.n_strata);
            it = a.rank_item[code];
            c0 = a.cptr[it];
            d = code < (uint32_t)a.n_hot ? 0u : (uint32_t)(a.cptr[it + 1] - c0);  // hot: no local positives
            if (code < (uint32_t)a.n_hot) it |= kLbHot;
        }
        item[g] = it;
        cp[g] = c0;
        cum[g + 1] = d;  // degrees; scanned below
        if (lock) lock[g] = 0;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the degrees (n_groups is ~10^2: one wave, chunks of 64)
        uint32_t run = 0;
        for (uint32_t g0 = 0; g0 < n_groups; g0 += kWave) {
            const uint32_t g = g0 + lane;
            uint32_t v = g < n_groups ? cum[g + 1] : 0u;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t t = __shfl_up(v, o, kWave);
                if (lane >= o) v += t;
            }
            if (g < n_groups) cum[g + 1] = run + v;
            run += __shfl(v, kWave - 1, kWave);
        }
        if (lane == 0) {
            cum[0] = 0;
            *sh_next_tile = 0;
            *sh_cold_mass = run;
            *sh_nslots = (n_groups && item[n_groups - 1] == -1) ? n_groups - 1 : n_groups;
        }
    }
    __syncthreads();
}

// draw `local` of bin c.b in epoch a.epoch: everything up to (and including) the request of the user id
template <bool POP>
__device__ __forceinline__ LdsBinDraw ldsbin_draw(const LdsBinArgs &a, const LdsBinCtx &c, uint32_t local, bool in_range) {
    LdsBinDraw d;
    d.in_range = in_range;
    uint32_t w[4];
    philox4x32_10(d.in_range ? local : 0u, c.b, a.epoch, 0x20u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
    const uint32_t r_pos = lemire_bounded2(w[0], w[1], c.n_draws, c.th_draw);
    uint32_t s_j, excl = 0, excl_lo = 0xffffffffu;   // the positive slot's interactions [excl_lo, excl_lo + excl) of the draw space
    if (r_pos < c.cold_mass) {
        uint32_t lo = 0, hi = c.n_slots;  // largest s with cum[s] <= r_pos
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (c.cum[mid] <= r_pos) lo = mid; else hi = mid;
        }
        d.u = a.cusers[c.cp[lo] + (int32_t)(r_pos - c.cum[lo])];
        d.ei = (int32_t)lo;
        // the negative: uniform over the OTHER slots of the bin (the positive itself is never a candidate; a bin of
        // one item has none and the draw is skipped by the membership test)
        s_j = c.n_slots > 1 ? lemire_bounded2(w[2], w[3], c.n_slots - 1, c.th_slot1) : 0u;
        if (c.n_slots > 1 && s_j >= lo) ++s_j;
        excl_lo = c.cum[lo];
        excl = c.cum[lo + 1] - excl_lo;
    } else {
        const uint32_t h = c.hot_lo + (r_pos - c.cold_mass);
        d.u = a.hot_u[h];
        d.ei = a.hot_i[h] | kLbHot;
        s_j = lemire_bounded2(w[2], w[3], c.n_slots, c.th_slot);  // a hot positive is dealt to any bin: all slots
    }
    if (POP) {
        // popularity-weighted negative: a second interaction of the bin's draw space, the positive slot's own
        // interactions left out (the reference's j == i draw is always skipped by has_non_zero and has probability
        // deg_i / nnz there; inside a bin it would be n_bins times as frequent).  Multiply-shift range reduction.
        const uint32_t m = c.n_draws - excl;
        uint32_t r_neg = (uint32_t)(((uint64_t)w[2] * m) >> 32);
        if (r_neg >= excl_lo) r_neg += excl;
        if (m == 0) {  // the bin holds nothing but the positive's interactions: no candidate, the membership test skips it
            d.j = c.item[d.ei] & ~kLbHot;
            d.ej = d.ei;
        } else if (r_neg < c.cold_mass) {
            uint32_t lo = 0, hi = c.n_slots;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (c.cum[mid] <= r_neg) lo = mid; else hi = mid;
            }
            d.j = c.item[lo];
            d.ej = (int32_t)lo;
        } else {
            d.j = a.hot_i[c.hot_lo + (r_neg - c.cold_mass)];
            d.ej = d.j | kLbHot;
        }
        return d;
    }
    const int32_t itj = c.item[s_j];
    d.j = itj & ~kLbHot;
    d.ej = itj < 0 ? itj : (int32_t)s_j;
    return d;
}

// the draws [d_lo, d_hi) of a bin that a launch covering [s_begin, s_begin + n) / nnz of the epoch makes, and the tile width:
// a tile = the draws one sampling pass makes (one per lane).  A launch that covers a chunk of an epoch holds few 64-draw
// tiles per wave and ends when its slowest wave has finished its last one: below 8 tiles per wave the tiles are 32 draws wide
// (half the lanes sample; the update steps, which dominate, are unchanged), which halves the tail.
__device__ __forceinline__ void ldsbin_launch_range(const LdsBinArgs &a, uint32_t n_draws, uint32_t n_waves, uint32_t &d_lo,
                                                    uint32_t &d_hi, uint32_t &tile_w, uint32_t &n_tiles) {
    d_lo = (uint32_t)(((unsigned __int128)n_draws * a.s_begin) / a.nnz);
    d_hi = a.s_begin + a.n >= a.nnz ? n_draws : (uint32_t)(((unsigned __int128)n_draws * (a.s_begin + a.n)) / a.nnz);
    tile_w = (d_hi - d_lo) < 8u * n_waves * kWave ? 32u : 64u;
    n_tiles = (d_hi - d_lo + tile_w - 1) / tile_w;
}

// CONV: conveyor launch (LdsBinArgs::conv_*): the workgroups cover bin ranges, the rows live in block buffers
// PRE: the launch trains the tiles ldsbin_presample_kernel has drawn (their valid triplets, compacted) instead of drawing them
template <int R, int UNR, bool POP = false, bool EXCH = false, int PF = 1, bool CONV = false, bool PRE = false>
__global__ __launch_bounds__(kLbBlock) void bpr_ldsbin_kernel(const LdsBinArgs a) {
    constexpr int G = kWave, KP = G * R, NREF = 2 * UNR;
    extern __shared__ float lb_smem[];
    float *const rows = lb_smem;
    float *const bias = rows + (size_t)a.cap * KP;
    int32_t *const item = reinterpret_cast<int32_t *>(bias + a.cap);
    int32_t *const cp = item + a.cap;
    uint32_t *const cum = reinterpret_cast<uint32_t *>(cp + a.cap);
    int *const lock = reinterpret_cast<int *>(cum + a.cap + 1);
    int32_t(*const stage)[3][kWave] = reinterpret_cast<int32_t(*)[3][kWave]>(lock + a.cap);
    const int wave = threadIdx.x >> 6, lane = lane_id();
    // waves of this workgroup: 16 where a bin owns a CU for the epoch, 8 where the bins of a large item table pass
    // through the LDS in many rounds and two workgroups share a CU (one loads its rows while the other trains)
    const uint32_t n_waves = blockDim.x >> 6;
    uint32_t b = blockIdx.x;
    const uint32_t nb = (uint32_t)a.n_bins;
    float *cvV = nullptr, *cvB = nullptr;   // conveyor: this bin's rows / biases in its block's buffer
    if (CONV) {
        const uint32_t r = blockIdx.x / (uint32_t)a.conv_bpb, o = blockIdx.x - r * (uint32_t)a.conv_bpb;
        b = (uint32_t)a.conv_first[r] + o;
        cvV = a.conv_rows[r] + (size_t)o * (size_t)a.cap * (size_t)a.k;
        cvB = a.conv_rows[r] + (size_t)a.conv_bpb * (size_t)a.cap * (size_t)a.k + (size_t)o * (size_t)a.cap;
    }
    const uint32_t n_groups = ((uint32_t)a.n_items + nb - 1) / nb;
#ifdef CORNAC_PROFILE
    if (a.wg_clock && threadIdx.x == 0) a.wg_clock[2 * b] = wall_clock64();
#endif
    // ---- the bin's items: slot g holds the item of group g dealt to this bin (the last group may have none) ----
    __shared__ uint32_t sh_nslots, sh_cold_mass, sh_next_tile;
    // resident exchange: parts done per boundary, exchanges each part has applied, one lock per part
    __shared__ uint32_t sh_ex_done[kLbMaxExchanges], sh_ex_applied[kLbWaves];
    __shared__ int sh_ex_lock[kLbWaves];
    if (EXCH) {
        if (threadIdx.x < kLbMaxExchanges) sh_ex_done[threadIdx.x] = 0;
        if (threadIdx.x < kLbWaves) {
            sh_ex_applied[threadIdx.x] = 0;
            sh_ex_lock[threadIdx.x] = 0;
        }
    }
    ldsbin_build_tables(a, b, nb, n_groups, item, cp, cum, lock, &sh_nslots, &sh_cold_mass, &sh_next_tile);
    const uint32_t n_slots = sh_nslots, cold_mass = sh_cold_mass;
    // the hot interactions [hot_off[b], hot_off[b + 1]) belong to this bin (ldsbin_level_kernel)
    const uint32_t hot_lo = a.hot_off[b], hot_share = a.hot_off[b + 1] - hot_lo;
    const uint32_t n_draws = n_slots ? cold_mass + hot_share : 0u;
    const uint32_t th_draw = n_draws ? lemire_thresh(n_draws) : 0u, th_slot = n_slots ? lemire_thresh(n_slots) : 0u,
                   th_slot1 = n_slots > 1 ? lemire_thresh(n_slots - 1) : 0u;
    bool inb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) inb[r] = lane + G * r < a.k;
    // ---- rows into LDS ----
    {
        // NL rows per wave in flight together (one row at a time is a chain of memory round trips: at 138 rows per bin and
        // 8 waves, 17 of them — a quarter of a passing bin's life)
        constexpr int NL = R <= 2 ? 4 : 2;
        for (uint32_t s0 = wave; s0 < n_slots; s0 += n_waves * NL) {
            float t[NL][R], tb[NL];
            int32_t its[NL];
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const uint32_t sq = s0 + (uint32_t)q * n_waves;
                its[q] = sq < n_slots ? item[sq] : -1;
                const size_t it = (size_t)(its[q] >= 0 ? its[q] : 0);
                const float *pv = CONV ? cvV + (size_t)(its[q] >= 0 ? sq : 0u) * a.k : a.V + it * a.k;
                const float *pb = CONV ? cvB + (its[q] >= 0 ? sq : 0u) : a.B + it;
#pragma unroll
                for (int r = 0; r < R; ++r) t[q][r] = (its[q] >= 0 && inb[r]) ? pv[lane + G * r] : 0.f;
                tb[q] = (its[q] >= 0 && lane == 0) ? *pb : 0.f;
            }
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                if (its[q] < 0) continue;  // (hot slot or past the end: wave-uniform)
                const uint32_t sq = s0 + (uint32_t)q * n_waves;
#pragma unroll
                for (int r = 0; r < R; ++r) rows[(size_t)sq * KP + lane + G * r] = t[q][r];
                if (lane == 0) bias[sq] = tb[q];
            }
        }
    }
    __syncthreads();
    unsigned int n_correct = 0, n_skipped = 0;
    if (!PRE && n_slots == 0 && wave == 0 && lane == 0 && a.s_begin == 0) n_skipped = cold_mass + hot_share;  // (degenerate: a bin without items; PRE: counted by the sampling launch)
    // this launch's share of the bin's draws: consecutive launches cover every draw of the epoch exactly once
    uint32_t d_lo, d_hi, tile_w, n_tiles;   // (ldsbin_launch_range: the draw of (bin, local index) does not depend on the tile width)
    ldsbin_launch_range(a, n_draws, n_waves, d_lo, d_hi, tile_w, n_tiles);
    const LdsBinCtx ctx{item, cp, cum, b, n_slots, cold_mass, hot_lo, n_draws, th_draw, th_slot, th_slot1};
    // Software pipeline over the wave's tiles (a CU runs only these 16 waves, so a wave has to keep its own memory
    // latencies covered): stage A = the draws of tile t + 2 with the load of the user id in flight, stage B = tile t + 1
    // with the membership word in flight, while the triplets of tile t are processed; inside a tile the user rows of
    // the next step are requested before the current step's atomics are issued (vmcnt retires in order: a load queued
    // behind the atomics would wait for their round trip to the memory side).
    typedef LdsBinDraw Draws;
    auto draw_tile = [&](uint32_t tile) {  // stage A: everything up to (and including) the request of the user id
        const uint32_t local = d_lo + tile * tile_w + lane;
        return ldsbin_draw<POP>(a, ctx, local, tile < n_tiles && (uint32_t)lane < tile_w && local < d_hi);
    };
    auto member_word = [&](const Draws &d) -> uint32_t {  // stage B: request the bitmap word of (u, j)
        return (a.bitmap && !LB_ABLATE(1)) ? a.bitmap[(size_t)d.u * a.bm_words + (d.j >> 5)] : 0u;
    };
    // without a bitmap (n_users x n_items bits would not fit): stage B requests the user's CSR row bounds instead, so that
    // the binary search of the membership test starts with them in registers
    auto member_bounds = [&](const Draws &d, int32_t &lo, int32_t &hi) {
        lo = hi = 0;
        if (!a.bitmap && !LB_ABLATE(1) && d.in_range) {
            lo = a.indptr[d.u];
            hi = a.indptr[d.u + 1];
        }
    };
    // tiles are claimed from a workgroup counter (a launch may hold only a few tiles per wave: a static deal would leave
    // waves idle for a whole tile at the end); which wave runs a tile does not change its draws
    auto claim_tile = [&]() -> uint32_t {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&sh_next_tile, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
    };
    // ---- resident exchange: the in-launch boundaries (see the header).  ex_per = tiles between two boundaries, ex_parts =
    // parts a boundary's duty is cut into; a bin with fewer tiles than exchanges publishes everything at the end
    const uint32_t ex_per = EXCH ? n_tiles / (uint32_t)a.ex.n_ex : 0u;
    const uint32_t ex_parts = ex_per < n_waves ? ex_per : n_waves;
    auto ex_landed_upto = [&](int from, int below) -> int {  // exchanges [from, result) have landed (they land in order)
        int e = from;
        if (lane == 0)
            while (e < below && __hip_atomic_load(a.ex.landed + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) ++e;
        return __builtin_amdgcn_readfirstlane(e);
    };
    auto ex_duty = [&](uint32_t t) {  // t: a tile this wave has just claimed
        if (!EXCH || ex_parts == 0u || t >= n_tiles) return;
        const uint32_t q = t / ex_per, part = t - q * ex_per;
        if (q == 0u || q >= (uint32_t)a.ex.n_ex || part >= ex_parts) return;
        const int e = (int)q - 1;
        // duties of one part are serialised (boundary e + 1's could start while boundary e's is still running)
        if (lane == 0)
            while (atomicCAS(&sh_ex_lock[part], 0, 1) != 0) __builtin_amdgcn_s_sleep(2);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int e_lo = (int)sh_ex_applied[part];
        const int e_hi = ex_landed_upto(e_lo, e);
        if (e_hi > e_lo) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the all-reduced buckets were written by other kernels
        // (profile builds, hogwild_flags bit 14: the part's rows in groups of NB with their loads in flight together —
        // 6.31-6.34 ms per epoch against 6.38-6.42 on the one-rank driver at the ML-20M shape, round 4's last call; it
        // passed the accounting tests once and is kept out of the shipped kernel until it has seen more boxes)
        constexpr int NB = R == 1 ? 4 : 2;  // rows in flight together (registers: ~12 R + 8 per row)
        if (!LB_ABLATE(64)) {
            for (uint32_t s = part; s < n_slots; s += ex_parts) {
                const int32_t it = item[s];
                if (it >= 0)
                    ex_row_duty<R>(a.ex, a.V, a.B, a.k, it, rows + (size_t)s * KP, bias + s, lock + s, e_lo, e_hi, e, lane, inb, a.counters + 3);
            }
        } else
        for (uint32_t s0 = part; s0 < n_slots; s0 += ex_parts * NB) {
            int32_t its[NB];
            float *lrow[NB], *lbias[NB];
            int *llock[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const uint32_t s = s0 + (uint32_t)q * ex_parts;
                const uint32_t sc = s < n_slots ? s : s0;
                const int32_t it = item[sc];
                its[q] = (s < n_slots && it >= 0) ? it : -1;
                lrow[q] = rows + (size_t)sc * KP;
                lbias[q] = bias + sc;
                llock[q] = lock + sc;
            }
            ex_rows_duty<R, NB>(a.ex, a.k, its, lrow, lbias, llock, e_lo, e_hi, e, lane, inb, a.counters + 3);
        }
        if (part == 0u)
            for (uint32_t hr = b; hr < (uint32_t)a.n_hot; hr += nb)
                ex_row_duty<R>(a.ex, a.V, a.B, a.k, a.rank_item[hr], nullptr, nullptr, nullptr, e_lo, e_hi, e, lane, inb, a.counters + 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's published rows have left for memory
        if (lane == 0) {
            sh_ex_applied[part] = (uint32_t)e_hi;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(&sh_ex_lock[part], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (atomicAdd(&sh_ex_done[e], 1u) == ex_parts - 1u)
                __hip_atomic_fetch_add(a.ex.arrive + e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };
    // ---- the valid triplets of a tile (compacted in stage[wave]): UNR triplets per step, the whole wave on one row at a time ----
    auto train_tile = [&](const int nvalid) __attribute__((always_inline)) {
        // ---- UNR triplets per step, the whole wave on one row at a time ----
        // the user rows of a step are requested PF steps ahead (PF register sets, used in turn)
        float u_nx[PF][UNR][R];
        int32_t tu_nx[PF][UNR];
        auto request_users = [&](float (&ub)[UNR][R], int32_t (&tub)[UNR], int t0) {
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                const int sl = t0 + q < nvalid ? t0 + q : (t0 < nvalid ? t0 : 0);
                tub[q] = __builtin_amdgcn_readfirstlane(stage[wave][0][sl]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    ub[q][r] = !inb[r] || LB_ABLATE(4) ? 0.f
                               : LB_ABLATE(8)          ? load_f32_fresh(a.U + (size_t)tub[q] * a.k + lane + G * r)
                                                       : __builtin_nontemporal_load(a.U + (size_t)tub[q] * a.k + lane + G * r);
            }
        };
        // one step: the UNR triplets [t0, t0 + UNR) of the tile, their user rows in the register set `ub`
        auto step = [&](float (&ub)[UNR][R], int32_t (&tub)[UNR], int t0) {
            float u_[UNR][R], v_[NREF][R], bv[NREF];
            float *pu[UNR];
            int32_t ref[NREF];
            bool act[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                act[q] = t0 + q < nvalid;
                const int sl = act[q] ? t0 + q : t0;
                ref[2 * q] = __builtin_amdgcn_readfirstlane(stage[wave][1][sl]);
                ref[2 * q + 1] = __builtin_amdgcn_readfirstlane(stage[wave][2][sl]);
                pu[q] = a.U + (size_t)tub[q] * a.k + lane;
#pragma unroll
                for (int r = 0; r < R; ++r) u_[q][r] = ub[q][r];
            }
            if (t0 + PF * UNR < nvalid) request_users(ub, tub, t0 + PF * UNR);  // a later step's user rows, ahead of this step's atomics
#pragma unroll
            for (int c = 0; c < NREF; ++c) {
                if (ref[c] < 0) {  // hot row: global memory (requesting it a step ahead with the user rows was measured: slower)
                    const int32_t it = ref[c] & ~kLbHot;
#pragma unroll
                    for (int r = 0; r < R; ++r) v_[c][r] = inb[r] ? load_f32_fresh(a.V + (size_t)it * a.k + lane + G * r) : 0.f;
                    bv[c] = load_f32_fresh(a.B + it);
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) v_[c][r] = rows[(size_t)ref[c] * KP + lane + G * r];
                    bv[c] = bias[ref[c]];
                }
            }
            float du[UNR][R], zq[UNR];
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                float part = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) part += u_[q][r] * (v_[2 * q][r] - v_[2 * q + 1][r]);
                // (profile builds, CORNAC_HIP_LDSBIN_X bit 0: no cross-lane sum, bit 1: no sigmoid — what they cost)
                const float score = (bv[2 * q] - bv[2 * q + 1]) + (LB_ABLATE(256) ? part : LB_ABLATE(1024) ? group_sum<G>(part) : wave_sum_dpp(part));
                const float z = LB_ABLATE(512) ? 0.5f + 1e-3f * score : sigmoid_neg_fast(score);
                zq[q] = z;
#pragma unroll
                for (int r = 0; r < R; ++r) du[q][r] = a.lr * (z * (v_[2 * q][r] - v_[2 * q + 1][r]) - a.reg * u_[q][r]);
                if (act[q] && lane == 0) n_correct += z < .5f ? 1u : 0u;
            }
            // user rows: any bin may hold interactions of a user -> device-scope atomics (exact)
#pragma unroll
            for (int q = 0; q < UNR; ++q) {
                if (!act[q] || LB_ABLATE(2)) continue;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (inb[r]) {
                        if (LB_ABLATE(8)) store_f32_agent(pu[q] + G * r, u_[q][r] + du[q][r]);   // (experiment: racy write-through RMW)
                        else if (LB_ABLATE(16)) pu[q][G * r] = u_[q][r] + du[q][r];                // (experiment: racy plain RMW)
                        else atomic_add_f32(pu[q] + G * r, du[q][r]);
                    }
            }
            // item rows: v += lr (+-z u - reg v) with v re-read under the row's lock (an LDS row belongs to this
            // workgroup only; the lock orders the 16 waves); hot rows by device-scope atomics on the loaded value
#pragma unroll
            for (int c = 0; c < NREF; ++c) {
                const int q = c >> 1;
                if (!act[q] || LB_ABLATE(2)) continue;
                const float zs = (c & 1) ? -zq[q] : zq[q];
                if (ref[c] < 0) {
                    const int32_t it = ref[c] & ~kLbHot;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (inb[r]) atomic_add_f32(a.V + (size_t)it * a.k + lane + G * r, a.lr * (zs * u_[q][r] - a.reg * v_[c][r]));
                    if (a.use_bias && lane == 0) atomic_add_f32(a.B + it, a.lr * (zs - a.reg * bv[c]));
                    continue;
                }
                const int s = ref[c];
                if (LB_ABLATE(32)) continue;   // (profile builds: no item-row update at all / 128: the update without the row lock)
                if (!EXCH && LB_ABLATE(2048)) {
                    // (experiment, profile builds: LDS float atomics — ds_add_f32 — instead of the locked read-modify-write.
                    // Measured at the ML-20M shape: 14.4 ms per epoch against 5.8: an LDS float atomic costs ~130 cycles per
                    // wave instruction, the lock's CAS round trip is the cheaper way to an exclusive row)
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        atomicAdd(rows + (size_t)s * KP + lane + G * r, a.lr * (zs * u_[q][r] - a.reg * v_[c][r]));
                    if (a.use_bias && lane == 0) atomicAdd(bias + s, a.lr * (zs - a.reg * bv[c]));
                    continue;
                }
                const bool owned = LB_ABLATE(128) ? false : lds_row_lock(&lock[s], lane, a.counters + 3);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float *pv = rows + (size_t)s * KP + lane + G * r;
                    const float v = *pv;
                    *pv = v + a.lr * (zs * u_[q][r] - a.reg * v);
                }
                if (a.use_bias && lane == 0) {
                    const float bb = bias[s];
                    bias[s] = bb + a.lr * (zs - a.reg * bb);
                }
                if (!LB_ABLATE(128)) lds_row_unlock(&lock[s], lane, owned);
            }
        };
        if (nvalid) request_users(u_nx[0], tu_nx[0], 0);
        if (PF == 2 && UNR < nvalid) request_users(u_nx[PF - 1], tu_nx[PF - 1], UNR);
        for (int t0 = 0; t0 < nvalid; t0 += PF * UNR) {
            step(u_nx[0], tu_nx[0], t0);
            if (PF == 2 && t0 + UNR < nvalid) step(u_nx[PF - 1], tu_nx[PF - 1], t0 + UNR);
        }
    };
    if constexpr (PRE) {
        // the tiles were drawn by ldsbin_presample_kernel: record pre_base[b] + tile holds the tile's valid triplets; the next
        // claimed tile's record is in flight while the current one trains
        const size_t pool0 = (size_t)a.pre_base[b];
        int32_t rec[3] = {0, 0, 0};
        uint32_t cnt = 0;
        auto fetch = [&](uint32_t t) {
            if (t < n_tiles) {
                const size_t o = pool0 + t;
                cnt = a.pre_cnt[o];
#pragma unroll
                for (int q = 0; q < 3; ++q) rec[q] = a.pre_rec[(o * 3 + q) * kWave + lane];
            }
        };
        uint32_t tB = n_tiles ? claim_tile() : 0u;
        fetch(tB);
        while (tB < n_tiles) {
            const int nvalid = __builtin_amdgcn_readfirstlane((int)cnt);
#pragma unroll
            for (int q = 0; q < 3; ++q) stage[wave][q][lane] = rec[q];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            tB = claim_tile();
            fetch(tB);
            train_tile(nvalid);
            __builtin_amdgcn_wave_barrier();
        }
    } else {
    uint32_t tB = n_tiles ? claim_tile() : 0u;
    Draws dB = n_tiles ? draw_tile(tB) : Draws{0, 0, 0, 0, false};
    if (n_tiles) ex_duty(tB);
    uint32_t tA = n_tiles ? claim_tile() : 0u;
    Draws dA = n_tiles ? draw_tile(tA) : dB;
    if (n_tiles) ex_duty(tA);
    uint32_t wordB = (n_tiles && dB.in_range) ? member_word(dB) : 0u;
    int32_t rowB_lo, rowB_hi;
    member_bounds(dB, rowB_lo, rowB_hi);
    while (tB < n_tiles) {
        // ---- tile `tile` leaves the pipeline: membership, compaction of the valid triplets ----
        bool skip = (wordB >> (dB.j & 31)) & 1u;
        if (!a.bitmap && !LB_ABLATE(1) && dB.in_range) skip = csr_row_contains(a.indices, rowB_lo, rowB_hi, dB.j);
        const bool valid = dB.in_range && !skip;
        const unsigned long long mask = __ballot(valid);
        n_skipped += (dB.in_range && !valid) ? 1u : 0u;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            stage[wave][0][pos] = dB.u;
            stage[wave][1][pos] = dB.ei;
            stage[wave][2][pos] = dB.ej;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nvalid = __popcll(mask);
        // ---- advance the pipeline: A -> B (its user ids have had a whole tile to arrive), new A ----
        dB = dA;
        tB = tA;
        wordB = dB.in_range ? member_word(dB) : 0u;
        member_bounds(dB, rowB_lo, rowB_hi);
        tA = claim_tile();
        dA = draw_tile(tA);
        ex_duty(tA);
        train_tile(nvalid);
        __builtin_amdgcn_wave_barrier();
    }
    }
    __syncthreads();
    if (EXCH) {
        // ---- the boundaries not met inside the loop: the last one (all of them for a bin with fewer tiles than
        // exchanges), by all waves; nobody trains any more, so no row lock.  Every row records how many exchanges it has
        // applied: ldsbin_exchange_flush_kernel applies the others after the last all-reduce.
        const int n_ex = a.ex.n_ex;
        const int landed_hi = ex_landed_upto(0, n_ex - 1);
        if (landed_hi > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int e = ex_parts ? n_ex - 1 : 0; e < n_ex; ++e) {
            const bool first = e == (ex_parts ? n_ex - 1 : 0);
            for (uint32_t s = wave; s < n_slots; s += n_waves) {
                const int32_t it = item[s];
                if (it < 0) continue;
                const int lo = ex_parts ? (int)sh_ex_applied[s % ex_parts] : 0;
                const int hi = ex_parts ? (landed_hi > lo ? landed_hi : lo) : 0;
                ex_row_duty<R>(a.ex, a.V, a.B, a.k, it, rows + (size_t)s * KP, bias + s, nullptr, first ? lo : hi, hi, e, lane, inb, a.counters + 3);
                if (lane == 0) a.ex.applied[it] = (unsigned int)hi;
            }
            if (wave == 0)
                for (uint32_t hr = b; hr < (uint32_t)a.n_hot; hr += nb) {
                    const int32_t it = a.rank_item[hr];
                    const int lo = ex_parts ? (int)sh_ex_applied[0] : 0;
                    const int hi = ex_parts ? (landed_hi > lo ? landed_hi : lo) : 0;
                    ex_row_duty<R>(a.ex, a.V, a.B, a.k, it, nullptr, nullptr, nullptr, first ? lo : hi, hi, e, lane, inb, a.counters + 3);
                    if (lane == 0) a.ex.applied[it] = (unsigned int)hi;
                }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_fetch_add(a.ex.arrive + e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // ---- rows back to the table ----
    for (uint32_t s = wave; s < n_slots; s += n_waves) {
        const int32_t it = item[s];
        if (it >= 0) {
            float *pv = CONV ? cvV + (size_t)s * a.k : a.V + (size_t)it * a.k;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (inb[r]) pv[lane + G * r] = rows[(size_t)s * KP + lane + G * r];
            if (lane == 0) *(CONV ? cvB + s : a.B + it) = bias[s];
        }
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
#ifdef CORNAC_PROFILE
    __syncthreads();
    if (a.wg_clock && threadIdx.x == 0) a.wg_clock[2 * b + 1] = wall_clock64();
#endif
}

// ---- pre-sampled launches --------------------------------------------------------------------------------------------
// What the ablation bits of the profile build showed at the ML-20M shape (profiles/r06_headline_ablation.log): of the 5.8 ms
// of an epoch, 2.3 ms remain when nothing is trained at all — the draws (Philox, two bounded draws, a binary search over the
// bin's degree scan), the dependent gather of the user id from the CSC segment and the membership word, all at the 16 waves
// per CU the LDS-resident rows allow.  None of that needs the bin's rows: ldsbin_presample_kernel makes the SAME draws (same
// function, same keys: ldsbin_draw) in a launch of its own at full occupancy — thousands of small workgroups whose memory
// latencies hide behind each other — applies the membership test and leaves, per tile, the valid triplets compacted in a
// record; the training launch (PRE instantiations) streams the records (three coalesced 256-byte loads per tile, the next
// tile's in flight) and only trains.  The triplets a bin trains in an epoch are the same set either way.
//
// pool layout: ldsbin_tilebase_kernel gives bin b the records [pre_base[b], pre_base[b + 1]) — an upper bound of its tiles
// from the deal's cold masses and hot runs (a bin without slots makes no draws but may have been dealt hot interactions).
struct LdsTileBaseArgs {
    const uint32_t *cold, *hot_off;
    uint32_t *base;       // [n_bins + 1]
    uint64_t s_begin, n, nnz;
    int32_t n_bins;
    uint32_t n_waves;
};

__global__ __launch_bounds__(kLbBlock) void ldsbin_tilebase_kernel(const LdsTileBaseArgs t) {   // one workgroup
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = lane_id();
    (void)wave;
    for (int32_t b0 = 0; b0 < t.n_bins; b0 += kLbBlock) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        uint32_t tiles = 0;
        if (b < t.n_bins) {
            const uint32_t n_draws = t.cold[b] + (t.hot_off[b + 1] - t.hot_off[b]);
            const uint32_t d_lo = (uint32_t)(((unsigned __int128)n_draws * t.s_begin) / t.nnz);
            const uint32_t d_hi = t.s_begin + t.n >= t.nnz ? n_draws : (uint32_t)(((unsigned __int128)n_draws * (t.s_begin + t.n)) / t.nnz);
            const uint32_t tile_w = (d_hi - d_lo) < 8u * t.n_waves * kWave ? 32u : 64u;
            tiles = (d_hi - d_lo + tile_w - 1) / tile_w;
        }
        // exclusive scan over the workgroup (wave scans + wave totals through LDS)
        __shared__ uint32_t wsum[kLbWaves];
        uint32_t v = tiles;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t u = __shfl_up(v, o, kWave);
            if (lane >= o) v += u;
        }
        if (lane == kWave - 1) wsum[threadIdx.x >> 6] = v;
        __syncthreads();
        uint32_t before = carry;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += wsum[w];
        if (b < t.n_bins) t.base[b] = before + v - tiles;
        __syncthreads();
        if (threadIdx.x == kLbBlock - 1) carry = before + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) t.base[t.n_bins] = carry;
}

constexpr int kLbPreBlock = 256;   // 4 waves per sampling workgroup
template <bool POP>
__global__ __launch_bounds__(kLbPreBlock) void ldsbin_presample_kernel(const LdsBinArgs a) {
    extern __shared__ float lb_smem[];
    int32_t *const item = reinterpret_cast<int32_t *>(lb_smem);
    int32_t *const cp = item + a.cap;
    uint32_t *const cum = reinterpret_cast<uint32_t *>(cp + a.cap);
    __shared__ uint32_t sh_nslots, sh_cold_mass, sh_next_tile;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const uint32_t b = blockIdx.x, nb = (uint32_t)a.n_bins;
    const uint32_t n_groups = ((uint32_t)a.n_items + nb - 1) / nb;
    ldsbin_build_tables(a, b, nb, n_groups, item, cp, cum, nullptr, &sh_nslots, &sh_cold_mass, &sh_next_tile);
    const uint32_t n_slots = sh_nslots, cold_mass = sh_cold_mass;
    const uint32_t hot_lo = a.hot_off[b], hot_share = a.hot_off[b + 1] - hot_lo;
    const uint32_t n_draws = n_slots ? cold_mass + hot_share : 0u;
    const uint32_t th_draw = n_draws ? lemire_thresh(n_draws) : 0u, th_slot = n_slots ? lemire_thresh(n_slots) : 0u,
                   th_slot1 = n_slots > 1 ? lemire_thresh(n_slots - 1) : 0u;
    unsigned int n_skipped = 0;
    if (n_slots == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.s_begin == 0) n_skipped = cold_mass + hot_share;  // (a bin without items)
    uint32_t d_lo, d_hi, tile_w, n_tiles;
    ldsbin_launch_range(a, n_draws, a.pre_waves, d_lo, d_hi, tile_w, n_tiles);
    const LdsBinCtx ctx{item, cp, cum, b, n_slots, cold_mass, hot_lo, n_draws, th_draw, th_slot, th_slot1};
    const size_t pool0 = (size_t)a.pre_base[b];
    const uint32_t stride = gridDim.y * (kLbPreBlock / kWave);
    for (uint32_t tile = blockIdx.y * (kLbPreBlock / kWave) + wave; tile < n_tiles; tile += stride) {
        const uint32_t local = d_lo + tile * tile_w + lane;
        const LdsBinDraw d = ldsbin_draw<POP>(a, ctx, local, (uint32_t)lane < tile_w && local < d_hi);
        bool skip;
        if (a.bitmap) {
            skip = d.in_range && ((a.bitmap[(size_t)d.u * a.bm_words + (d.j >> 5)] >> (d.j & 31)) & 1u);
        } else {
            skip = d.in_range && csr_row_contains(a.indices, a.indptr[d.u], a.indptr[d.u + 1], d.j);
        }
        const bool valid = d.in_range && !skip;
        const unsigned long long mask = __ballot(valid);
        n_skipped += (d.in_range && !valid) ? 1u : 0u;
        const size_t o = pool0 + tile;
        if (valid) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));
            a.pre_rec[(o * 3 + 0) * kWave + pos] = d.u;
            a.pre_rec[(o * 3 + 1) * kWave + pos] = d.ei;
            a.pre_rec[(o * 3 + 2) * kWave + pos] = d.ej;
        }
        if (lane == 0) a.pre_cnt[o] = (uint32_t)__popcll(mask);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_skipped += __shfl_xor(n_skipped, o, kWave);
    if (lane == 0 && n_skipped) atomicAdd(&a.counters[1], (unsigned long long)n_skipped);
}

// ---- per-epoch deal bookkeeping: the bins' cold masses, then the hot runs that level them ----
struct LdsDealArgs {
    const int32_t *cptr, *rank_item;
    uint32_t *mass;      // [n_bins] zero on entry (ldsbin_level_kernel re-zeroes it)
    uint32_t *cold_out;  // [n_bins] the epoch's cold masses (inspection / tests)
    uint32_t *hot_off;   // [n_bins + 1]
    uint32_t key;
    int32_t n_items, n_bins, n_hot, n_hot_inter, n_strata, hot_cost_x16;
};

__global__ __launch_bounds__(kLbBlock) void ldsbin_mass_kernel(const LdsDealArgs a) {
    const uint32_t nb = (uint32_t)a.n_bins, ni = (uint32_t)a.n_items;
    const uint32_t n_groups = (ni + nb - 1) / nb;
    for (uint32_t p = blockIdx.x * kLbBlock + threadIdx.x; p < ni; p += gridDim.x * kLbBlock) {
        const uint32_t g = p / nb, o = p - g * nb;
        const uint32_t code = ldsbin_deal_rank(p, a.key, nb, ni, n_groups, (uint32_t)a.n_strata);
        if (code < (uint32_t)a.n_hot) continue;
        const int32_t it = a.rank_item[code];
        const uint32_t d = (uint32_t)(a.cptr[it + 1] - a.cptr[it]);
        if (d) atomicAdd(&a.mass[(o + ldsbin_rot(g, a.key, nb)) % nb], d);
    }
}

// Levels the bins with the hot interactions.  A cold draw costs 16 units, a hot one hot_cost_x16: with the level L =
// the largest value for which sum_b floor(max(0, L - 16 cold_b) / hot_cost_x16) <= n_hot_inter, bin b takes that many
// hot interactions and the remainder goes one each to the bins b = 0, 1, ... (round robin).  hot_cost_x16 = 0: an even
// split.  Integer arithmetic only: oracle/cornac_oracle.c restates it.  One workgroup.
__host__ __device__ inline uint64_t ldsbin_level_share(uint64_t level, uint32_t cold, uint32_t cost_x16) {
    const uint64_t t = 16ull * cold;
    return level > t ? (level - t) / cost_x16 : 0ull;
}

__global__ __launch_bounds__(kLbBlock) void ldsbin_level_kernel(const LdsDealArgs a) {
    __shared__ unsigned long long sh_red[kLbWaves];
    __shared__ unsigned long long sh_val;
    const uint32_t nb = (uint32_t)a.n_bins, H = (uint32_t)a.n_hot_inter, c16 = (uint32_t)a.hot_cost_x16;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    auto block_sum = [&](unsigned long long v) -> unsigned long long {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        __syncthreads();
        if (lane == 0) sh_red[wave] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int w = 0; w < kLbWaves; ++w) t += sh_red[w];
            sh_val = t;
        }
        __syncthreads();
        return sh_val;
    };
    uint64_t level = 0;
    if (c16 && H) {
        unsigned long long tot = 0;  // bounds the level: no bin is heavier than all of them together
        for (uint32_t b = threadIdx.x; b < nb; b += kLbBlock) tot += a.mass[b];
        uint64_t lo = 0, hi = 16ull * block_sum(tot) + (uint64_t)c16 * ((uint64_t)H + 1ull);
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            unsigned long long part = 0;
            for (uint32_t b = threadIdx.x; b < nb; b += kLbBlock) part += ldsbin_level_share(mid, a.mass[b], c16);
            if (block_sum(part) <= (unsigned long long)H) lo = mid; else hi = mid - 1;
        }
        level = lo;
    }
    unsigned long long part = 0;
    if (c16 && H)
        for (uint32_t b = threadIdx.x; b < nb; b += kLbBlock) part += ldsbin_level_share(level, a.mass[b], c16);
    const uint64_t rest = (uint64_t)H - block_sum(part);
    // exclusive scan over the bins in index order (chunks of the block width)
    __shared__ uint32_t sh_scan[kLbBlock];
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kLbBlock) {
        const uint32_t b = b0 + threadIdx.x;
        uint32_t share = 0, cold = 0;
        if (b < nb) {
            cold = a.mass[b];
            share = (uint32_t)((c16 && H) ? ldsbin_level_share(level, cold, c16) : 0ull) + (uint32_t)(rest / nb) +
                    (b < (uint32_t)(rest % nb) ? 1u : 0u);
        }
        sh_scan[threadIdx.x] = share;
        __syncthreads();
        for (int o = 1; o < kLbBlock; o <<= 1) {
            const uint32_t t = (int)threadIdx.x >= o ? sh_scan[threadIdx.x - o] : 0u;
            __syncthreads();
            sh_scan[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nb) {
            a.hot_off[b + 1] = run + sh_scan[threadIdx.x];
            a.cold_out[b] = cold;
            a.mass[b] = 0;
        }
        run += sh_scan[kLbBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.hot_off[0] = 0;
}

// Conveyor: the (bin, slot) layout of a deal, written out — slot_item[b cap + g] = the item dealt to slot g of bin b (-1: the
// last group has none for this bin), item_slot[i] = b cap + g of item i.  The block buffers hold their rows in this order
// (LdsBinArgs::conv_rows); the epoch-boundary re-deal of cornac_amd/dist.py moves every row from its slot under the old key to
// its slot under the new one.
__global__ __launch_bounds__(kLbBlock) void ldsbin_layout_kernel(const int32_t *__restrict__ rank_item, uint32_t key, int32_t n_items,
                                                                  int32_t n_bins, int32_t cap, int32_t n_strata,
                                                                  int32_t *__restrict__ slot_item, int32_t *__restrict__ item_slot) {
    const uint32_t nb = (uint32_t)n_bins, ni = (uint32_t)n_items;
    const uint32_t n_groups = (ni + nb - 1) / nb;   // == cap
    const uint64_t total = (uint64_t)n_groups * nb;
    for (uint64_t p = (uint64_t)blockIdx.x * kLbBlock + threadIdx.x; p < total; p += (uint64_t)gridDim.x * kLbBlock) {
        const uint32_t g = (uint32_t)(p / nb), o = (uint32_t)(p - (uint64_t)g * nb);
        const uint32_t b = (o + ldsbin_rot(g, key, nb)) % nb;
        const size_t slot = (size_t)b * (size_t)cap + g;
        if (p < ni) {
            const int32_t it = rank_item[ldsbin_deal_rank((uint32_t)p, key, nb, ni, n_groups, (uint32_t)n_strata)];
            if (slot_item) slot_item[slot] = it;
            if (item_slot) item_slot[it] = (int32_t)slot;
        } else if (slot_item) {
            slot_item[slot] = -1;
        }
    }
}

// bitmap[u][j >> 5] bit (j & 31) = 1 iff (u, j) is an interaction
__global__ __launch_bounds__(kBlock) void ldsbin_bitmap_kernel(const int32_t *__restrict__ user_ids,
                                                                const int32_t *__restrict__ indices, int64_t nnz,
                                                                int bm_words, uint32_t *__restrict__ bitmap) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nnz) return;
    const int32_t j = indices[t];
    atomicOr(&bitmap[(size_t)user_ids[t] * bm_words + (j >> 5)], 1u << (j & 31));
}

// ---- resident exchange: what runs beside / after the epoch's launch -----------------------------------------------
// After the last all-reduce of the epoch has landed: every row receives the exchanges its owner did not apply inside
// the launch (applied[i] .. n_ex - 1), on the table and on the base alike.  One wave per row.
__global__ __launch_bounds__(kBlock) void ldsbin_exchange_flush_kernel(const LdsBinExchange x, float *__restrict__ V,
                                                                        float *__restrict__ B, int32_t n_items, int k) {
    const int lane = lane_id();
    const size_t nk = (size_t)x.nt * (size_t)k;
    const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t it = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); it < n_items; it += waves) {
        const int e_lo = (int)x.applied[it];
        for (int e = e_lo; e < x.n_ex; ++e) {
            // an exchange whose all-reduce never landed (the communication stream gave up waiting: its flag stays 0) is not
            // applied — its bucket is incomplete; exchanges land in order
            if (x.landed && __hip_atomic_load(x.landed + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) break;
            const float *S = x.bucket + (size_t)e * (size_t)x.bucket_stride;
            const float *K = x.keep + (size_t)e * (size_t)x.keep_stride;
            float n2 = 0.f;
            if (x.rule != 0) {
                for (int f = lane; f < k; f += kWave) n2 += S[(size_t)it * k + f] * S[(size_t)it * k + f];
                n2 = group_sum<kWave>(n2);
            }
            const float fv = ex_rule_factor(x.rule, S[nk + (size_t)x.nt + it], n2);
            for (int f = lane; f < k; f += kWave) {
                const size_t o = (size_t)it * k + f;
                const float c = S[o] * fv - K[o];
                V[o] += c;
                x.base[o] += c;
            }
            if (lane == 0) {
                const float sb = S[nk + it];
                const float cb = sb * ex_rule_factor(x.rule, S[nk + 2 * (size_t)x.nt + it], sb * sb) - K[nk + it];
                B[it] += cb;
                x.base[nk + it] += cb;
            }
        }
    }
}

// The communication stream's side of the hand-shake: one lane polls an arrival counter until it reaches `target` (the
// epoch's launch bumps it and never waits for anything, so this ends), or gives up after `timeout_ticks` of the 100 MHz
// wall clock and raises *err — a would-be hang becomes an error the host reports.
__global__ void stream_wait_counter_kernel(const unsigned int *__restrict__ counter, unsigned int target,
                                           unsigned int *__restrict__ err, long long timeout_ticks) {
    if (threadIdx.x != 0) return;
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;  // an earlier wait gave up: do not wait again
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < target) {
        if ((long long)(wall_clock64() - t0) > timeout_ticks) {
            __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        __builtin_amdgcn_s_sleep(32);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// unless != nullptr and *unless != 0 (an earlier stream_wait_counter_kernel gave up): the flag is NOT set
__global__ void stream_set_flag_kernel(unsigned int *__restrict__ flag, unsigned int value, const unsigned int *__restrict__ unless) {
    if (threadIdx.x != 0) return;
    if (unless && __hip_atomic_load(unless, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A stand-in for the kernel a ring all-reduce runs on THIS rank when the process group has one member (RCCL then
// launches nothing): n_workgroups workgroups — a collective's channel count, not a copy kernel's full grid — stream `n`
// floats through (read src cyclically over src_n floats, write dst cyclically over dst_n), i.e. the 2 (N - 1) / N x
// bucket bytes a rank receives, reduces and forwards.  One-GPU measurements of the multi-GPU drivers then carry the
// collective's HBM traffic and its workgroups' share of the CUs (bench.py legs.dist_tax).
__global__ __launch_bounds__(512) void stream_ring_standin_kernel(const float *__restrict__ src, long long src_n,
                                                                   float *__restrict__ dst, long long dst_n, long long n) {
    // 16-byte accesses, 8 of them in flight per thread (a collective's kernels keep the links busy; one 4-byte load in
    // flight per thread would make the stand-in latency-bound at a few GB/s and say nothing about contention)
    const long long n4 = n >> 2, s4 = src_n >> 2, d4 = dst_n >> 2;
    const v4f *s = reinterpret_cast<const v4f *>(src);
    v4f *d = reinterpret_cast<v4f *>(dst);
    const long long stride = (long long)gridDim.x * 512;
    long long i = (long long)blockIdx.x * 512 + threadIdx.x;
    long long si = i % s4, di = i % d4;
    const long long sstep = stride % s4, dstep = stride % d4;
    for (; i + 7 * stride < n4; i += 8 * stride) {
        v4f t[8];
        long long sj = si;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            t[q] = __builtin_nontemporal_load(s + sj);
            sj += sstep;
            if (sj >= s4) sj -= s4;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            __builtin_nontemporal_store(t[q], d + di);
            di += dstep;
            if (di >= d4) di -= d4;
        }
        si = sj;
    }
    for (; i < n4; i += stride) {
        __builtin_nontemporal_store(__builtin_nontemporal_load(s + si), d + di);
        si += sstep; if (si >= s4) si -= s4;
        di += dstep; if (di >= d4) di -= d4;
    }
}

}  // namespace chip

/*
 * cornac_hip.h — C ABI of libcornac_hip.so, the MI355X (gfx950) backend for the
 * embedding-SGD + scoring hot path of PreferredAI/cornac.
 *
 * The reference has no FFI: its plug-in boundary is four Cython call sites.
 * Every entry point below names the reference interface it replaces (paths are
 * relative to the reference repository root).  The reference-side bindings a
 * maintainer would add are shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++ exceptions cross the boundary; every function returns an
 *     int status (0 = CORNAC_HIP_OK) and cornac_hip_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - host buffers are caller-owned; device buffers are library-owned unless a
 *     *_bind_device call hands in caller-owned device pointers (used by the
 *     multi-GPU driver so torch.distributed/RCCL can all-reduce them in place);
 *   - calls on one handle are not re-entrant (one HIP stream per handle);
 *     different handles may be driven from different threads / devices;
 *   - all calls block until the device work is complete unless stated otherwise.
 */
#ifndef CORNAC_HIP_H_
#define CORNAC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORNAC_HIP_OK 0
#define CORNAC_HIP_ERR_INVALID 1   /* bad argument (message says which)            */
#define CORNAC_HIP_ERR_HIP 2       /* a HIP runtime call failed                    */
#define CORNAC_HIP_ERR_NO_DEVICE 3 /* no gfx950 device visible                     */
#define CORNAC_HIP_ERR_UNSUPPORTED 4

/* Execution mode.
 * DETERMINISTIC reproduces the reference's seeded run (seed != None forces
 * num_threads = 1, cornac/models/bpr/recom_bpr.pyx:132-133, recom_mf.py:124-125):
 * every update observes all earlier ones, in the reference's sample order.
 * HOGWILD is the throughput mode, the counterpart of the reference's racy
 * multi-thread path (num_threads > 1, recom_bpr.pyx:228-267, backend_cpu.pyx:62). */
#define CORNAC_HIP_MODE_DETERMINISTIC 0
#define CORNAC_HIP_MODE_HOGWILD 1

/* Negative-item population of the triplet sampler. */
#define CORNAC_HIP_NEG_UNIFORM 0    /* BPR : neg_item_ids = arange(num_items)  (recom_bpr.pyx:186)  */
#define CORNAC_HIP_NEG_POPULARITY 1 /* WBPR: neg_item_ids = X.indices          (recom_wbpr.pyx:135) */

const char *cornac_hip_last_error(void);
const char *cornac_hip_version(void);
int cornac_hip_device_count(int *count);
/* name (<=255 chars), CU count and HBM bytes of a device */
int cornac_hip_device_info(int device, char *name, int name_len, int *compute_units, int64_t *hbm_bytes);
/* Memory-system calibration of the box a benchmark runs on (bench.py reports it beside the scale leg, whose
 * throughput differs between boxes): over two scratch buffers of `bytes` each, out3 = {device-to-device copy GB/s
 * (read + written), streaming read GB/s, random 512-byte row gather GB/s} */
int cornac_hip_device_probe(int device, int64_t bytes, double *out3);

/* ------------------------------------------------------------------------- *
 * BPR / WBPR trainer.
 * Replaces: BPR._fit_sgd(rng_pos, rng_neg, num_threads, user_ids, item_ids,
 *           neg_item_ids, indptr, U, V, B) -> (correct, skipped)
 *           cornac/models/bpr/recom_bpr.pyx:208-269, its caller loop
 *           BPR.fit :188-201 and WBPR.fit cornac/models/bpr/recom_wbpr.pyx:127-142,
 *           the sampler RNGVector recom_bpr.pyx:54-62 and has_non_zero :46-51.
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_bpr *cornac_hip_bpr_t;

/* CSR interaction matrix = train_set.matrix (int32 indptr[n_users+1], int32
 * indices[nnz], sorted per row — cornac/data/dataset.py:226-235).  U is
 * [total_users, k], V is [total_items, k], B is [total_items] like BPR._init
 * (recom_bpr.pyx:145-152); n_users/n_items are the TRAIN counts used by the
 * sampler. */
int cornac_hip_bpr_create(cornac_hip_bpr_t *out, int device, int64_t n_users, int64_t n_items,
                          int64_t total_users, int64_t total_items, int k, const int32_t *indptr,
                          const int32_t *indices, int64_t nnz);
int cornac_hip_bpr_destroy(cornac_hip_bpr_t h);

/* host -> device / device -> host copies of the factor tables (fp32, C order).
 * Any pointer may be NULL to skip that table. */
int cornac_hip_bpr_set_factors(cornac_hip_bpr_t h, const float *U, const float *V, const float *B);
int cornac_hip_bpr_get_factors(cornac_hip_bpr_t h, float *U, float *V, float *B);

/* float64 tables.  `_fit_sgd` is a fused-type (`floating`) function (recom_bpr.pyx:211-214): a model given float64
 * U / V / Bi through init_params trains in double, every local of the step included (:219-224).  set_factors_f64 puts
 * the handle into that state (all three tables together; set_factors puts it back), fit_epochs_f64 runs the SEQUENTIAL
 * semantics (the deterministic engine with the mt19937 streams of seed_mt19937; lr / reg as doubles) — there is no
 * float64 throughput kernel: an unseeded float64 model is trained by this engine too (cornac_amd/bpr.py). */
int cornac_hip_bpr_set_factors_f64(cornac_hip_bpr_t h, const double *U, const double *V, const double *B);
int cornac_hip_bpr_get_factors_f64(cornac_hip_bpr_t h, double *U, double *V, double *B);
int cornac_hip_bpr_fit_epochs_f64(cornac_hip_bpr_t h, int n_epochs, double lr, double reg, int use_bias, int neg_population,
                                  int64_t *correct, int64_t *skipped);

/* Use caller-owned device buffers (same shapes) instead of the library's. */
int cornac_hip_bpr_bind_device(cornac_hip_bpr_t h, float *dU, float *dV, float *dB);
int cornac_hip_bpr_device_ptrs(cornac_hip_bpr_t h, float **dU, float **dV, float **dB);
/* Swap caller-owned item tables for other caller-owned ones WITHOUT synchronising the handle's stream (bind_device waits
 * for it): work already enqueued keeps its pointers, later work sees the new ones.  For drivers that move the item
 * table between launches — the ring conveyor of cornac_amd/dist.py binds the block that has just arrived. */
int cornac_hip_bpr_rebind_items(cornac_hip_bpr_t h, float *dV, float *dB);
/* run the handle's work on a caller-provided hipStream_t (NULL = the handle's own); waits for the previous stream */
int cornac_hip_bpr_set_stream(cornac_hip_bpr_t h, void *hip_stream);
/* the same without waiting for the work already queued on the previous stream: for callers that alternate between two
 * streams and order them with events themselves (cornac_amd/dist.py:RowShardedBprTrainer, stages A / B) */
int cornac_hip_bpr_switch_stream(cornac_hip_bpr_t h, void *hip_stream);

/* Deterministic-mode sampler state = the two boost::random::mt19937 engines of
 * RNGVector(1, ...) (recom_bpr.pyx:188-191): pass the ALREADY-DERIVED 32-bit
 * mt19937 seeds (RandomState(seed_a).randint(2**31)).  shared_stream != 0 is
 * WBPR's single generator used for both draws (recom_wbpr.pyx:131).  The
 * streams persist across fit_epochs calls exactly like the reference's
 * RNGVector objects persist across epochs. */
int cornac_hip_bpr_seed_mt19937(cornac_hip_bpr_t h, uint32_t mt_seed_pos, uint32_t mt_seed_neg, int shared_stream);
/* Hogwild-mode sampler state: counter-based Philox4x32-10 keyed by `seed`;
 * the epoch counter persists across calls. */
int cornac_hip_bpr_seed_hogwild(cornac_hip_bpr_t h, uint64_t seed);

/* Popularity-weighted negatives (CORNAC_HIP_NEG_POPULARITY) draw the item of a uniformly chosen entry of `neg_item_ids`
 * (recom_wbpr.pyx:135-139: neg_item_ids = X.indices, the handle's own interactions by default).  A handle that holds only
 * a SLICE of the users (multi-GPU) can be given the population of the whole matrix instead: items[n], any multiset of
 * train item ids whose multiplicities are (proportional to) the global item degrees; n = 0 restores the default.  With a
 * caller's population the popularity draw runs in the fused kernel (the LDS-bin form weights by the handle's own CSC). */
int cornac_hip_bpr_set_negative_population(cornac_hip_bpr_t h, const int32_t *items, int64_t n);

/* The bits of hogwild_flags (explained at cornac_hip_bpr_fit_epochs below). */
#define CORNAC_HIP_HOG_PLAIN_STORES 1    /* bit0: plain (racy, non-atomic, XCD-incoherent) row stores, not fp32 atomics */
#define CORNAC_HIP_HOG_VEC4_LAYOUT 2     /* bit1: the float4-per-lane row layout                                        */
#define CORNAC_HIP_HOG_NO_OWNERSHIP 4    /* bit2: no user-row ownership (all rows atomic)                               */
#define CORNAC_HIP_HOG_DENSE_BIAS 8      /* bit3: the dense bias table, not one bias per 128-byte line                  */
/* bit4: (k in 33..64) the four sampling lanes 4g..4g+3 share one negative item and its row gets ONE combined atomic
 * update — a different joint distribution of the draws than the reference's, kept as a measured experiment */
#define CORNAC_HIP_HOG_SHARE_NEG 16
/* bit5 (32): reserved.  No kernel reads it; like every set bit below the form field it keeps the call out of the
 * LDS-bin, XCD-strata and binned forms, so a word that carries it runs the fused kernel as if it did not. */
/* bit6: the segmented ("binned") item-update path (k in 33..256); taken only when it is the one bit set among bits 0..6 */
#define CORNAC_HIP_HOG_BINNED 64
#define CORNAC_HIP_HOG_FUSED_OPT_OUT 128 /* bit7: opts out of the LDS-bin / XCD-strata forms, nothing else              */
#define CORNAC_HIP_HOG_ABLATE_MASK 0xff00 /* bits 8..15: ablation switches of the SGD kernels (profile builds only)     */
#define CORNAC_HIP_HOG_ABLATE_SHIFT 8
#define CORNAC_HIP_HOG_FORM_MASK 0xf0000  /* bits 16..19: the form field                                                */
#define CORNAC_HIP_HOG_FORM_SHIFT 16
#define CORNAC_HIP_FORM_AUTO (0 << CORNAC_HIP_HOG_FORM_SHIFT)
#define CORNAC_HIP_FORM_FUSED (1 << CORNAC_HIP_HOG_FORM_SHIFT)
#define CORNAC_HIP_FORM_STRATA (2 << CORNAC_HIP_HOG_FORM_SHIFT)
#define CORNAC_HIP_FORM_LDSBIN (3 << CORNAC_HIP_HOG_FORM_SHIFT)

/* Run n_epochs epochs of nnz samples each.  correct/skipped accumulate the
 * reference's per-epoch counters over the epochs run (either may be NULL).
 * hogwild_flags (0 = default) is the word of CORNAC_HIP_HOG_* bits above.  Its form field selects the form of a
 * hogwild call: CORNAC_HIP_FORM_AUTO, CORNAC_HIP_FORM_FUSED (every item-row update a device-scope fp32 atomic; also
 * CORNAC_HIP_HOG_FUSED_OPT_OUT), CORNAC_HIP_FORM_STRATA (csrc/bpr_strata.inc: 8 launches per epoch, an item row is
 * touched by one XCD per launch and updated by plain read-modify-write like the reference's threads),
 * CORNAC_HIP_FORM_LDSBIN (csrc/bpr_ldsbin.inc: the item rows of a bin live in one CU's LDS for the epoch, exact
 * updates, user rows by atomics).  Automatic = LDS bins when the item table fits the LDS in at most max_rounds rounds
 * with at least min_candidates items per bin, else XCD strata for item tables of >= 2^20 rows, else the fused kernel
 * (the whole decision: the table over hog_form in csrc/bpr.hip).  A chunk of an epoch (hogwild_enqueue) runs in the
 * same form: an LDS-bin launch takes its share of every bin's draws, an XCD-strata chunk runs the partition phases that
 * begin inside it.  Popularity negatives (WBPR) have the LDS-bin form too — the negative is the item of a second
 * interaction drawn from the bin's own draw space, hot items dealt to every bin — but not the XCD-strata one; every
 * switch (any of bits 0..15) runs the fused kernel, or the binned path where CORNAC_HIP_HOG_BINNED says so. */
int cornac_hip_bpr_fit_epochs(cornac_hip_bpr_t h, int n_epochs, float lr, float reg, int use_bias, int neg_population,
                              int mode, int hogwild_flags, int64_t *correct, int64_t *skipped);
/* Same, but only enqueues `n_samples` hogwild samples (sample counter and
 * epoch continue) on the handle's stream and returns without synchronising;
 * counters are added into device memory and fetched by ..._sync.  Used by the
 * multi-GPU driver to interleave training chunks with RCCL reductions. */
int cornac_hip_bpr_hogwild_enqueue(cornac_hip_bpr_t h, int64_t n_samples, float lr, float reg, int use_bias,
                                   int neg_population, int hogwild_flags);
int cornac_hip_bpr_sync(cornac_hip_bpr_t h, int64_t *correct, int64_t *skipped);

/* Test hooks of the deterministic sampler: draw `n` values from stream 0/1
 * (boost uniform_int_distribution<long>(0, hi), uniform_int_distribution.hpp:188-227). */
int cornac_hip_bpr_debug_draw(cornac_hip_bpr_t h, int stream, uint64_t hi, int64_t n, int64_t *out);
/* Test hook of the hogwild sampler's user-row ownership: *n_waves receives the
 * width W of the persistent grid (0 when ownership is not used for this
 * handle); wave_ptr[W+1], own_u[nnz] (negative = shared heavy user, stored as
 * ~u), own_i[nnz] receive the tables when non-NULL. */
int cornac_hip_bpr_debug_ownership(cornac_hip_bpr_t h, int64_t *n_waves, int64_t *wave_ptr, int32_t *own_u,
                                   int32_t *own_i);
/* Tuning and inspection of the XCD-strata form.  strata_config: the hot item rows (atomic updates) are the most
 * popular ranks that are touched at least hot_min_mult_x100 / 100 times as often as the average row and together
 * receive at most hot_permille / 1000 of the item-row touches (defaults 200, 120); the item partitions are re-dealt
 * every rehash_period epochs (default 1).  strata_stats: out4 = {hot rows (-1: tables not built yet), workgroup
 * launches that were surplus on their XCD since create (an XCD handed more than an eighth of a launch: those fell back
 * to atomics; parts are claimed at run time from HW_REG_XCC_ID, so blockIdx placement does not matter), bucket builds, grid
 * width in waves (0: the strata form has not run)}.  debug_strata (test hook): deals the partitions of `epoch` and
 * returns the bucket offsets sptr[8 W + 1], the bucketed records rec_u / rec_i [nnz] (rec_i: bit 31 = hot row),
 * rank_item [n_items] (popularity rank -> item) and the epoch key; any pointer may be NULL. */
int cornac_hip_bpr_strata_config(cornac_hip_bpr_t h, int hot_permille, int hot_min_mult_x100, int rehash_period);
/* Inside cornac_hip_bpr_fit_epochs the XCD-strata form trains on packed item records (row + its bias line = one random
 * location per item, csrc/bpr_strata.inc); every other entry point gets the dense V / B back first.  enable = 1 lets the
 * chunk API (cornac_hip_bpr_hogwild_enqueue) keep the records from call to call as well — for a caller that touches the
 * (bound) dense table between chunks only through cornac_hip_bpr_table_delta_begin / _step / _finish, which then work on
 * the records, and reads it after cornac_hip_bpr_sync, which writes the records back (the multi-GPU driver of
 * cornac_amd/dist.py with the dense exchange).  Default 0. */
int cornac_hip_bpr_chunk_records(cornac_hip_bpr_t h, int enable);
int cornac_hip_bpr_strata_stats(cornac_hip_bpr_t h, int64_t *out4);
int cornac_hip_bpr_debug_strata(cornac_hip_bpr_t h, uint32_t epoch, int64_t *sptr, int32_t *rec_u, int32_t *rec_i,
                                int32_t *rank_item, uint32_t *key);
/* Tuning and inspection of the LDS-bin form.  ldsbin_config: an item is hot (rows in global memory under atomics, its
 * interactions dealt to all bins) when its degree exceeds hot_x1000 / 1000 of a bin's share nnz / bins (default 75;
 * passing bins: of nnz / (4 x CUs) — a quarter of what one of the 2 x CUs concurrent slots draws per epoch);
 * the form is used when every bin holds at least min_candidates items (default 48: the negative of a draw comes from
 * the positive's bin) and the table fits in max_rounds rounds of one bin per CU (default 4: "resident bins", a bin owns
 * its CU for the epoch).  ldsbin_pass_config: "passing bins" for item tables beyond that — the table passes through the
 * LDS once per epoch in as many rounds as it takes, `waves` waves (4 / 8 / 16; default 8) and at most lds_kb KiB
 * (default 64: two workgroups per CU) per bin, used when an epoch draws at least min_draws_x100 / 100 interactions per
 * item row (default 200) and for launches of at least a quarter of an epoch; enable = 0 switches the regime off
 * (automatic then falls through to XCD strata / the fused kernel).  ldsbin_stats: out8 =
 * {bins (0: the shape does not use the form), LDS rows per bin, hot items, their interactions, bitmap words per user
 * (0: CSR binary search), dynamic LDS bytes per workgroup, row-lock spins that hit their bound since create (0
 * unless there is a bug: fetched with the epoch counters; the resident exchange's row duties count here too), threads
 * per workgroup (1024 resident bins, 64 x waves passing bins)}. */
int cornac_hip_bpr_ldsbin_config(cornac_hip_bpr_t h, int hot_x1000, int min_candidates, int max_rounds);
int cornac_hip_bpr_ldsbin_pass_config(cornac_hip_bpr_t h, int enable, int waves, int lds_kb, int min_draws_x100);
int cornac_hip_bpr_ldsbin_stats(cornac_hip_bpr_t h, int64_t *out8);
/* The per-epoch deal of the LDS-bin form (csrc/bpr_ldsbin.inc, ldsbin_deal_rank).  deal_config: the popularity ranks
 * are permuted (epoch-keyed) inside strata of ~strata_groups * bins consecutive ranks before they are cut into the
 * groups of `bins` items that are dealt one item to each bin (default 16; 1 = the groups are cut from the static rank
 * order, so two items of one group never share a bin); the hot interactions are dealt to the bins in runs that level
 * the bins' work with a hot draw priced at hot_cost_x16 / 16 cold draws (default 32; 0 = an even split).
 * debug_ldsbin_deal (test hook): deals epoch `epoch` of hogwild seed `seed` and returns bin_of_item [n_items],
 * cold_mass [bins] (interactions of the bin's own items), hot_off [bins + 1] (the bin's run of the hot list) and the
 * shuffled hot list hot_u / hot_i [hot interactions]; any pointer may be NULL. */
int cornac_hip_bpr_ldsbin_deal_config(cornac_hip_bpr_t h, int strata_groups, int hot_cost_x16);
int cornac_hip_bpr_debug_ldsbin_deal(cornac_hip_bpr_t h, uint64_t seed, uint32_t epoch, int32_t *bin_of_item,
                                     uint32_t *cold_mass, uint32_t *hot_off, int32_t *hot_u, int32_t *hot_i);
/* HIP-event timing of the hogwild SGD kernel launches, recorded on the handle's
 * stream: returns the summed duration and count of the launches recorded since
 * the previous call, then enables/disables recording for the following ones. */
int cornac_hip_bpr_kernel_timing(cornac_hip_bpr_t h, int enable, double *total_ms, int64_t *launches);
/* time spent (ms) in the last fit_epochs call: [0] sampler, [1] host level
 * scheduling, [2] SGD kernels, [3] total */
int cornac_hip_bpr_last_timing(cornac_hip_bpr_t h, double *ms4);

/* ------------------------------------------------------------------------- *
 * Building blocks of the row-sharded item table (multi-GPU regime 2): the same
 * _fit_sgd step (cornac/models/bpr/recom_bpr.pyx:208-269) cut into sample / fetch / apply / push
 * because the item rows of a triplet live on other GPUs.  All pointers are DEVICE pointers; all
 * launches go to the handle's stream.  Driven by cornac_amd/dist.py:RowShardedBprTrainer.
 * ------------------------------------------------------------------------- */
/* draws n_draws (u, i, j) with the hogwild sampler (continues the handle's sample counter); a draw whose
 * negative is a positive of u ("skipped", recom_bpr.pyx:236-238) is written as u = i = j = -1 */
int cornac_hip_bpr_sample_triplets(cornac_hip_bpr_t h, int64_t n_draws, int neg_population, int32_t *d_u,
                                   int32_t *d_i, int32_t *d_j);
/* BPR update of the handle's U rows and of STAGED item rows: d_slot_i/j index rows of d_rows [n_slots, k]
 * and d_bias [n_slots * bias_stride]; entries with d_u < 0 are ignored */
int cornac_hip_bpr_apply_triplets(cornac_hip_bpr_t h, const int32_t *d_u, const int32_t *d_slot_i,
                                  const int32_t *d_slot_j, int64_t n, float *d_rows, float *d_bias, int bias_stride,
                                  float lr, float reg, int use_bias);
/* The same two steps through the hogwild kernel's user-row ownership (k in 33..256): emit_triplets runs the owned
 * sampler of the fused kernel and writes the triplets of tile t of wave w at ((t * waves + w) * 64 + lane) — u with
 * bit 30 set for a shared (heavy) user, u = i = j = -1 for a skipped or padding slot; *n_slots (a multiple of
 * waves * 64, at most what staged_slots(n_draws) returns, <= slots_cap) is the array length written.  apply_staged
 * takes the same arrays with i / j replaced by staging-table slots: every user row is again touched by one wave only
 * (plain loads/stores, atomics only on the staged item rows), exactly the fused kernel's update.
 * staged_slots returns 0 when the shape has no owned kernel (use sample_triplets / apply_triplets). */
int cornac_hip_bpr_staged_slots(cornac_hip_bpr_t h, int64_t n_draws, int64_t *n_slots);
int cornac_hip_bpr_emit_triplets(cornac_hip_bpr_t h, int64_t n_draws, int neg_population, int32_t *d_u, int32_t *d_i,
                                 int32_t *d_j, int64_t slots_cap, int64_t *n_slots);
int cornac_hip_bpr_apply_staged(cornac_hip_bpr_t h, const int32_t *d_u, const int32_t *d_slot_i, const int32_t *d_slot_j,
                                int64_t n_slots, float *d_rows, float *d_bias, int bias_stride, float lr, float reg,
                                int use_bias);
/* De-duplication of a micro-batch's item ids without a sort.  Owner-major index of item i:
 * g(i) = (i % world) * rows_per_rank + i / world.  shard_mark sets d_mark[g] = 1 for the items of every valid triplet
 * (d_mark: int32 [world * rows_per_rank], zeroed by the caller); the caller scans it (inclusive); shard_slots writes
 * slot = d_scan[g] - 1 per triplet side (-1 for skipped draws); shard_uniq writes the request lists
 * d_uniq_local[d_scan[g] - 1] = g % rows_per_rank, one contiguous run per owner. */
int cornac_hip_bpr_shard_mark(cornac_hip_bpr_t h, const int32_t *d_i, const int32_t *d_j, int64_t n, int world,
                              int64_t rows_per_rank, int32_t *d_mark);
int cornac_hip_bpr_shard_slots(cornac_hip_bpr_t h, const int32_t *d_i, const int32_t *d_j, int64_t n, int world,
                               int64_t rows_per_rank, const int32_t *d_scan, int32_t *d_slot_i, int32_t *d_slot_j);
int cornac_hip_bpr_shard_uniq(cornac_hip_bpr_t h, const int32_t *d_mark, const int32_t *d_scan, int64_t n_rows,
                              int64_t rows_per_rank, int32_t *d_uniq_local);
/* d_table[d_ids[r], :] += (d_now[r, :] - d_before[r, :]) * (d_scale ? d_scale[r] : 1)  (atomic): the owner's side of
 * a push — d_before is the row as the owner sent it, d_now the row as the requester returned it */
int cornac_hip_bpr_scatter_diff_rows(cornac_hip_bpr_t h, float *d_table, const int32_t *d_ids, int64_t n, int width,
                                     const float *d_now, const float *d_before, const float *d_scale);
/* d_out[r, :] = d_table[d_ids[r], :] and d_table[d_ids[r], :] += d_delta[r, :] (atomic), rows of `width` floats */
int cornac_hip_bpr_gather_rows(cornac_hip_bpr_t h, const float *d_table, const int32_t *d_ids, int64_t n, int width,
                               float *d_out);
int cornac_hip_bpr_scatter_add_rows(cornac_hip_bpr_t h, float *d_table, const int32_t *d_ids, int64_t n, int width,
                                    const float *d_delta);
/* Replicated item table (multi-GPU regime 1): the elementwise passes around the all-reduce of the table deltas.
 * flat = [V (n_items*k) | B (n_items)] is the replica the kernels train on, base its value at the last exchange.
 * begin : bucket = [flat - base | V rows touched (n_items) | biases touched (n_items)], local = copy of flat - base
 * finish: (after bucket was sum-all-reduced) R = delta / sqrt(max(touching ranks, 1)) per row; flat += R - local;
 *         base += R */
int cornac_hip_bpr_table_delta_begin(cornac_hip_bpr_t h, const float *d_flat, const float *d_base, int64_t n_items,
                                     int k, float *d_bucket, float *d_local);
int cornac_hip_bpr_table_delta_finish(cornac_hip_bpr_t h, float *d_flat, float *d_base, const float *d_bucket,
                                      const float *d_local, int64_t n_items, int k);
/* finish of the previous exchange followed by begin of the next one, in one pass (adjacent in the overlapped schedule) */
int cornac_hip_bpr_table_delta_step(cornac_hip_bpr_t h, float *d_flat, float *d_base, const float *d_bucket_prev,
                                    const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local);
/* The three passes with the reconciliation rule as an argument (op: 0 = begin, 1 = finish, 2 = step; rule: 0 = "sqrt",
 * 1 = "align", described below), on the handle's stream and on its packed records where it keeps them: the regime-1
 * driver takes "align" when it exchanges less than a few times per epoch (sparse item sides: DESIGN.md 5). */
int cornac_hip_bpr_table_delta(cornac_hip_bpr_t h, int op, int rule, float *d_flat, float *d_base, const float *d_bucket_prev,
                               const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local);
/* The same passes for a caller without a BPR handle (the MF driver): op & 15: 0 = begin, 1 = finish, 2 = step, on
 * `hip_stream` of `device`; begin ignores the *_prev pointers, finish the next-exchange pointers.  op >> 4 selects the
 * reconciliation rule: 0 = "sqrt" (the one above: per-row slots of the bucket = touched flags, R = S / sqrt(count)),
 * 1 = "align" (per-row slots = |delta row|^2 of this rank, R = S * min(1, sum of the slots / |S|^2): the sum of
 * orthogonal deltas, the mean of identical ones — MF's default, cornac_amd/dist.py ItemTableReplica). */
int cornac_hip_table_delta(int op, int device, void *hip_stream, float *d_flat, float *d_base, const float *d_bucket_prev,
                           const float *d_local_prev, int64_t n_items, int k, float *d_bucket, float *d_local);
/* Resident exchange: multi-GPU regime 1 for the LDS-bin form WITHOUT chunk launches (the reference has no counterpart:
 * BPR._fit_sgd, recom_bpr.pyx:208-269, is one process; the update it distributes is :252-265).  ONE launch per epoch
 * publishes the item-table deltas of this rank at n_exchanges points and applies the all-reduced sums of the earlier
 * points as soon as their `landed` flag is set — the launch never waits for the collective (csrc/bpr_ldsbin.inc).
 *   d_base     [nt k + nt], nt = total_items: as in the table_delta passes; table - base = steps not yet published
 *   d_buckets  exchange e at + e * bucket_stride floats: [dV (nt k) | dB (nt) | wV (nt) | wB (nt)], all-reduced in place by
 *              the caller; d_keeps exchange e at + e * keep_stride: this rank's own [dV | dB]
 *   d_arrive   [n_exchanges] zero on entry; reaches *n_arrivals (the launch's workgroups) when bucket e is complete
 *   d_landed   [n_exchanges] zero on entry; the caller sets [e] != 0 after the all-reduce of bucket e (in order)
 *   d_applied  [n_items] out: row i has applied the exchanges [0, d_applied[i])
 * The caller's communication stream runs, for e = 0 .. n_exchanges-1: cornac_hip_stream_wait_counter(d_arrive + e,
 * *n_arrivals) -> all-reduce of bucket e -> cornac_hip_stream_set_flag(d_landed + e); when the last one has landed,
 * cornac_hip_bpr_resident_flush (on the handle's stream) applies what the launch did not (d_landed: the landed exchanges only).  The bound tables
 * (cornac_hip_bpr_bind_device) are the replica.  cornac_hip_bpr_resident_exchange_bins: *n_bins = the launch's
 * workgroup count, 0 when this shape / these flags do not take the LDS-bin form (use hogwild_enqueue chunks then). */
int cornac_hip_bpr_resident_exchange_bins(cornac_hip_bpr_t h, int neg_population, int hogwild_flags, int *n_bins);
int cornac_hip_bpr_epoch_resident_enqueue(cornac_hip_bpr_t h, float lr, float reg, int use_bias, int neg_population,
                                          int hogwild_flags, int n_exchanges, int rule, float *d_base, float *d_buckets,
                                          int64_t bucket_stride, float *d_keeps, int64_t keep_stride, uint32_t *d_arrive,
                                          const uint32_t *d_landed, uint32_t *d_applied, int *n_arrivals);
int cornac_hip_bpr_resident_flush(cornac_hip_bpr_t h, int n_exchanges, int rule, float *d_base, const float *d_buckets,
                                  int64_t bucket_stride, const float *d_keeps, int64_t keep_stride,
                                  const uint32_t *d_applied, const uint32_t *d_landed);
/* Conveyor layout of the LDS-bin form — multi-GPU regime 2 ("V rows owned by ..." — here the item table is
 * sharded by row into n_blocks blocks that rotate over the ranks, cornac_amd/dist.py BinConveyorBprTrainer).  No reference
 * counterpart (cornac is one process); a launch computes recom_bpr.pyx:231-267 for the draws of its bins.
 *   conveyor_setup   plans the bins as n_blocks equal ranges (block B = the bins [B bpb, (B + 1) bpb) of the epoch's deal: a
 *                    block's ITEMS change with the deal key like any bin's, so every (positive, negative) pair of items can
 *                    meet), no hot items; rank_item [n_items]: the popularity order every rank of the fit agrees on (NULL: the
 *                    handle's own interactions'); deal_seed: shared by the ranks (the draws keep the handle's hogwild seed);
 *                    release_item_tables != 0 frees the handle's own V / B (the rows live in the caller's block buffers).
 *                    Out: *n_bins, *bins_per_block, *cap (slots per bin).  A block buffer is [bpb cap k rows | bpb cap biases]
 *                    floats, row (bin - first bin of the block) cap + slot.
 *   conveyor_layout  on the handle's stream: d_slot_item [n_bins cap] = the item at (bin, slot) under the deal of layout_epoch
 *                    (-1: none), d_item_slot [n_items] = its inverse (either may be NULL)
 *   conveyor_enqueue one launch on the handle's stream: all of this handle's draws of `epoch` whose positive lies in the blocks
 *                    first_block[0 .. n_ranges) (distinct; n_ranges <= 8), rows read from / written to d_rows[r]; the deal is
 *                    that of layout_epoch (the caller re-deals the buffers when it changes).  Counters: cornac_hip_bpr_sync. */
int cornac_hip_bpr_conveyor_setup(cornac_hip_bpr_t h, int n_blocks, const int32_t *rank_item, uint64_t deal_seed,
                                  int release_item_tables, int *n_bins, int *bins_per_block, int *cap);
int cornac_hip_bpr_conveyor_layout(cornac_hip_bpr_t h, uint32_t layout_epoch, int32_t *d_slot_item, int32_t *d_item_slot);
int cornac_hip_bpr_conveyor_enqueue(cornac_hip_bpr_t h, uint32_t epoch, uint32_t layout_epoch, int n_ranges,
                                    const int32_t *first_block, float *const *d_rows, float lr, float reg, int use_bias,
                                    int neg_population, int hogwild_flags);
/* on `hip_stream` of `device`: wait until *d_counter >= target (after timeout_ms: *d_error = 1 and the stream moves on;
 * every later wait on the same d_error returns at once); set *d_flag = value unless d_unless != NULL and *d_unless != 0.
 * The resident exchange passes its d_error as d_unless: a bucket that was all-reduced incomplete never gets its landed
 * flag, so neither the launch nor cornac_hip_bpr_resident_flush (d_landed) applies it; the caller reports d_error. */
int cornac_hip_stream_wait_counter(int device, void *hip_stream, const uint32_t *d_counter, uint32_t target,
                                   uint32_t *d_error, int timeout_ms);
int cornac_hip_stream_set_flag(int device, void *hip_stream, uint32_t *d_flag, uint32_t value, const uint32_t *d_unless);
/* Measurement aid (no reference counterpart): what a ring all-reduce costs THIS rank's memory system and CUs when the
 * process group has a single member and RCCL therefore launches nothing — n_workgroups workgroups of 512 threads stream
 * n_floats floats from d_src (read cyclically over src_floats) to d_dst (written cyclically over dst_floats) on
 * hip_stream.  cornac_amd/dist.py puts it where the collective sits when asked to emulate a world of N ranks
 * (n_floats = 2 (N - 1) / N x the bucket). */
int cornac_hip_stream_ring_standin(int device, void *hip_stream, const float *d_src, int64_t src_floats, float *d_dst,
                                   int64_t dst_floats, int64_t n_floats, int n_workgroups);

/* ------------------------------------------------------------------------- *
 * VEBPR (view-enhanced BPR) on the same handle.
 * Replaces: VEBPR._fit_sgd_viewloss(rng_pos, rng_view, rng_neg, ..., U, V)
 *           cornac/models/bpr/recom_vebpr.pyx:211-337 and its caller loop :189-207.
 * The handle's CSR is the purchase matrix; set_views adds the view matrix
 * (train_set.view_matrix: views minus purchases, sorted rows,
 * cornac/data/dataset.py:1400-1440).  No item biases.
 * ------------------------------------------------------------------------- */
int cornac_hip_bpr_set_views(cornac_hip_bpr_t h, const int32_t *view_indptr, const int32_t *view_indices,
                             int64_t nnz_view);
/* third mt19937 engine (rng_view, recom_vebpr.pyx:192); call after cornac_hip_bpr_seed_mt19937 */
int cornac_hip_bpr_seed_view_stream(cornac_hip_bpr_t h, uint32_t mt_seed_view);
int cornac_hip_vebpr_fit_epochs(cornac_hip_bpr_t h, int n_epochs, float lr, float reg, float alpha, int mode,
                                int64_t *correct, int64_t *skipped);
/* The float64 instantiation of the same fused-type function (recom_vebpr.pyx:219 `floating[:, :] U, floating[:, :] V`,
 * reached by float64 init_params): tables set with cornac_hip_bpr_set_factors_f64 (its bias table is not used), all
 * locals of the step in double, sequential semantics (the three mt19937 streams) only, like cornac_hip_bpr_fit_epochs_f64. */
int cornac_hip_vebpr_fit_epochs_f64(cornac_hip_bpr_t h, int n_epochs, double lr, double reg, double alpha, int64_t *correct,
                                    int64_t *skipped);
/* Hogwild mode (the reference's prange over samples, recom_vebpr.pyx:211-337) gives every wave of the grid a fixed set of
 * users (k > 32 and enough interactions for one 64-sample tile per wave): positives come from the wave's own users, so
 * an exclusive user's row has one writer and is updated by plain load / store; the three item rows keep fp32 atomics.
 * OR this bit into `mode` for the all-atomic form (diagnostics, A/B); vebpr_hogwild_form reports what the last hogwild
 * epoch ran (1 = user-row ownership). */
#define CORNAC_HIP_VEBPR_NO_OWNERSHIP 0x100
int cornac_hip_vebpr_hogwild_form(cornac_hip_bpr_t h, int *owned);

/* ------------------------------------------------------------------------- *
 * MMMF (maximum-margin matrix factorisation) on the same handle.
 * Replaces: MMMF._fit_sgd(rng_pos, rng_neg, ..., U, V, B)
 *           cornac/models/mmmf/recom_mmmf.pyx:103-160 under BPR's caller loop
 *           (cornac/models/bpr/recom_bpr.pyx:189-206).
 * BPR's sampler under the soft-margin ranking loss: a triplet whose score is
 * already positive is counted in `correct` and updates nothing (:145-147); a
 * violator (score <= 0) moves its three rows and, always, its two biases
 * (:150-158; the loop has no use_bias switch).  Uniform negatives only.
 * Every entry point refuses, with an error code and a cornac_hip_last_error
 * text: a handle with a negative population set, a conveyor-configured handle,
 * the table type the call is not for, n_epochs < 0, an unknown mode, and a mode
 * whose sampler has not been seeded.
 * ------------------------------------------------------------------------- */
/* n_epochs epochs of recom_mmmf.pyx:126-158 over float32 tables; mode: CORNAC_HIP_MODE_DETERMINISTIC (after
 * cornac_hip_bpr_seed_mt19937: the two mt19937 streams, sequential semantics, bit-faithful) or CORNAC_HIP_MODE_HOGWILD
 * (after cornac_hip_bpr_seed_hogwild: the reference's num_threads > 1 prange, :123-126).  correct / skipped are summed
 * over the call, as in cornac_hip_bpr_fit_epochs. */
int cornac_hip_mmmf_fit_epochs(cornac_hip_bpr_t h, int n_epochs, float lr, float reg, int mode, int64_t *correct,
                               int64_t *skipped);
/* The float64 instantiation of the same fused-type function (recom_mmmf.pyx:103-106 `floating[:, :] U, ... floating[:] B`,
 * locals :113-116), reached by float64 init_params: tables set with cornac_hip_bpr_set_factors_f64, sequential semantics
 * only, like cornac_hip_bpr_fit_epochs_f64. */
int cornac_hip_mmmf_fit_epochs_f64(cornac_hip_bpr_t h, int n_epochs, double lr, double reg, int64_t *correct,
                                   int64_t *skipped);
/* One hogwild launch of n_samples iterations of recom_mmmf.pyx:126-158 at the handle's current sample offset (the
 * numbering of BPR's unowned fused form), asynchronous; cornac_hip_bpr_sync collects the counters. */
int cornac_hip_mmmf_hogwild_enqueue(cornac_hip_bpr_t h, int64_t n_samples, float lr, float reg);

/* ------------------------------------------------------------------------- *
 * Matrix factorisation trainer.
 * Replaces: backend_cpu.fit_sgd(rid, cid, val, U, V, Bu, Bi, lr, reg, mu,
 *           max_iter, num_threads, use_bias, early_stop, verbose)
 *           cornac/models/mf/backend_cpu.pyx:35-97 (called from
 *           MF._fit_cpu, cornac/models/mf/recom_mf.py:189-209).
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_mf *cornac_hip_mf_t;

/* rid/cid are the int64 COO arrays of train_set.uir_tuple in stored order, val fp32. */
int cornac_hip_mf_create(cornac_hip_mf_t *out, int device, int64_t n_users, int64_t n_items, int k,
                         const int64_t *rid, const int64_t *cid, const float *val, int64_t nnz);
int cornac_hip_mf_destroy(cornac_hip_mf_t h);
int cornac_hip_mf_set_factors(cornac_hip_mf_t h, const float *U, const float *V, const float *Bu, const float *Bi);
int cornac_hip_mf_get_factors(cornac_hip_mf_t h, float *U, float *V, float *Bu, float *Bi);
/* Runs up to max_iter epochs; loss_per_epoch[e] = 0.5 * sum(err^2) (may be NULL);
 * early_stop: stop when |loss - last_loss| < 1e-5 (backend_cpu.pyx:89-93).
 * epochs_run receives the number of epochs executed. */
int cornac_hip_mf_fit(cornac_hip_mf_t h, int max_iter, float lr, float reg, float mu, int use_bias, int early_stop,
                      int mode, float *loss_per_epoch, int *epochs_run);
/* Form of the last deterministic epoch of cornac_hip_mf_fit: *form = 1 the persistent dataflow launch (k <= 256 and
 * nnz >= 4096), 2 one launch per level of the row-conflict schedule (also after a refused cooperative launch), 0 none
 * yet; *own_user = 1 if the dataflow launch's waves owned the user rows, 0 if the item rows (0 unless *form is 1).
 * Either pointer may be NULL. */
int cornac_hip_mf_det_form(cornac_hip_mf_t h, int *form, int *own_user);
/* Form of the hogwild MF epoch: 0 = automatic, 1 = the fused kernel (user rows owned by waves, item rows by fp32
 * atomics), 2 = the block rotation (csrc/mf_blocks.inc: item bins in the CUs' LDS, user blocks rotating among the 32
 * workgroups of an XCD, 8 launches x 32 barrier-separated sub-rounds per epoch; no atomics, every update applied exactly
 * once).  Automatic = the block rotation for k in 33..256, >= 256 items and >= 2^22 ratings on a 256-CU / 8-XCD device.
 * 3 = the STEP form, for handles that hold one step of a larger schedule — few item rows, most ratings of the launch in
 * flight at once — such as the per-block handles of dist.MfBlockRotationTrainer: the fused kernel launched with only ~4
 * ratings in flight per item row, and item rows that still take more than 32 concurrent updates trained through copies
 * merged after the launch, AT ANY SIZE (forms 0..2 split rows only from 2^20 ratings on: an item holding > 0.1 % of them).
 * Choose it before the handle's first epoch.
 * hogwild_stats: out4 = {form of the last epoch (1 / 2, 0: none yet), tiles of the block schedule, LDS rows per bin,
 * 1 if the rotation gave up once (workgroup placement / barrier bound) and the handle went back to the fused kernel}. */
int cornac_hip_mf_hogwild_form(cornac_hip_mf_t h, int form);
int cornac_hip_mf_hogwild_stats(cornac_hip_mf_t h, int64_t *out4);
/* Read-only test hooks of the hogwild forms; both copy from the handle's tables and change nothing.
 * debug_split: *n_split receives the number of item rows that train through copies and *n_virtual the number of copies
 * (0 and 0 before the first hogwild launch, or when no row is split); split_item[n_split] and split_ptr[n_split + 1]
 * (copies of split item j = virtual rows [split_ptr[j], split_ptr[j + 1]), ids n_items + v) receive the tables when non-NULL.
 * debug_ownership: *n_waves receives the width W of the persistent grid when the LAST hogwild launch ran the fused kernel
 * with user-row ownership (0 otherwise); wave_ptr[W + 1], own_u[nnz] (negative = shared heavy user, stored as ~u) and
 * own_i[nnz] (ids >= n_items name copies of split rows) receive the tables when non-NULL. */
int cornac_hip_mf_debug_split(cornac_hip_mf_t h, int64_t *n_split, int64_t *n_virtual, int32_t *split_item, int32_t *split_ptr);
int cornac_hip_mf_debug_ownership(cornac_hip_mf_t h, int64_t *n_waves, int64_t *wave_ptr, int32_t *own_u, int32_t *own_i);
/* One-shot form with the reference's exact argument list (host buffers, in place). */
int cornac_hip_mf_fit_sgd(int device, const int64_t *rid, const int64_t *cid, const float *val, int64_t nnz, float *U,
                          float *V, float *Bu, float *Bi, int64_t n_users, int64_t n_items, int k, float lr, float reg,
                          float mu, int max_iter, int use_bias, int early_stop, int mode, float *loss_per_epoch,
                          int *epochs_run);
/* Multi-GPU driver surface (no counterpart in the reference; cornac_amd/dist.py ShardedMfTrainer): every rank holds the
 * ratings of its own users (U, Bu local), the item side [V | Bi] is replicated in caller-owned device memory and
 * reconciled by the caller between slices.  bind_items: train into caller-owned V (n_items x k) and Bi (n_items);
 * set_stream: run on a caller stream (NULL = the handle's own); epoch_enqueue: ratings [nnz*part/n_parts,
 * nnz*(part+1)/n_parts) of the stored order, hogwild semantics, NO host synchronisation (n_parts = 1: the whole epoch in
 * the form cornac_hip_mf_fit would pick); sync: wait, and return the sum of squared errors enqueued since the last sync. */
int cornac_hip_mf_bind_items(cornac_hip_mf_t h, float *dV, float *dBi);
/* bind_users: train into caller-owned U (n_users x k) and Bu (n_users) — cornac_amd/dist.py MfBlockRotationTrainer: the handles
 * of a rank's item blocks (each created over the rank's ratings of one block, item ids local to it) share the rank's user side
 * and are bound, step by step, to whichever buffer holds their block. */
int cornac_hip_mf_bind_users(cornac_hip_mf_t h, float *dU, float *dBu);
int cornac_hip_mf_set_stream(cornac_hip_mf_t h, void *hip_stream);
int cornac_hip_mf_epoch_enqueue(cornac_hip_mf_t h, int part, int n_parts, float lr, float reg, float mu, int use_bias);
int cornac_hip_mf_sync(cornac_hip_mf_t h, double *sq_err_sum);
int cornac_hip_mf_kernel_timing(cornac_hip_mf_t h, int enable, double *total_ms, int64_t *launches);
int cornac_hip_mf_last_timing(cornac_hip_mf_t h, double *ms4);

/* PMF on the same handle: the reference's sequential per-rating SGD with an RMSProp cache, in float64.
 * Replaces: pmf.pmf_linear / pmf.pmf_non_linear(uid, iid, rat, n_users, n_items, n_ratings, k, n_epochs, lambda_reg,
 *           learning_rate, gamma, init_params, verbose, seed)
 *           cornac/models/pmf/cython/pmf.pyx:55-111 and :115-173 (called from PMF.fit,
 *           cornac/models/pmf/recom_pmf.py:143-176); the handle's `val` are the ratings as the reference passes them
 *           (float32, rescaled to [0, 1] by the caller for the non-linear variant).
 * Ratings run in the stored order, as on the reference's single thread: one persistent dataflow launch per epoch (k <= 256
 * and nnz >= 4096; for k <= 32 several ready ratings per wave pass, in lane groups of pow2 >= k lanes), else one launch per
 * level of the row-conflict schedule.  U and V come out bit-identical to the sequential loop's; the loss is summed in
 * another order.  The float32 MF state of the handle is untouched. */
#define CORNAC_HIP_PMF_LINEAR 0
#define CORNAC_HIP_PMF_NON_LINEAR 1
/* float64 U [n_users,k], V [n_items,k]; zeroes the RMSProp caches (the reference allocates them per fit call) */
int cornac_hip_mf_pmf_set_factors(cornac_hip_mf_t h, const double *U, const double *V);
int cornac_hip_mf_pmf_get_factors(cornac_hip_mf_t h, double *U, double *V);
/* n_epochs sequential epochs over the stored order; caches persist across calls until set_factors;
 * loss_per_epoch [n_epochs] may be NULL; lr / reg / gamma are the reference's float arguments */
int cornac_hip_mf_pmf_fit(cornac_hip_mf_t h, int n_epochs, float lr, float reg, float gamma, int variant, double *loss_per_epoch);
/* 1 = dataflow launch, 2 = level schedule, 0 = none yet; *group = ratings per wave pass of the last epoch */
int cornac_hip_mf_pmf_form(cornac_hip_mf_t h, int *form, int *group);

/* NMF on the same handle: multiplicative updates in float32, tables of their own (the MF and PMF state of the handle is
 * untouched, and an MF or PMF fit leaves these alone).
 * Replaces: NMF._fit_sgd(rid, cid, val, user_counts, item_counts, U, V, Bu, Bi)
 *           cornac/models/nmf/recom_nmf.pyx:182-267 (called from NMF.fit, :162-180, with the CSR of train_set.matrix).
 * The handle's ratings must be stored by user (rid non-decreasing), as the reference's CSR is: cornac_hip_mf_nmf_fit
 * refuses any other order.  One epoch, every float32 operation separately rounded:
 *   r_pred = ((mu + Bu[u]) + Bi[i]) + U[u,0] V[i,0] + ... (index order); error = r - r_pred            (:228-232)
 *   use_bias: Bu[u] += lr (error - lambda_bu Bu[u]); Bi[i] += lr (error - lambda_bi Bi[i]), in stored order (:236-238)
 *   U_num += r V, U_den += r_pred V, V_num += r U, V_den += r_pred U from zero                          (:241-245)
 *   U_den += count_u lambda_u U + 1e-9f; U *= U_num / U_den for the users, then the items (a row without ratings
 *   becomes zero)                                                                                       (:248-259)
 *   loss = sum error^2 + lambda_u sum U^2 + lambda_v sum V^2 over the pre-update tables, float32 terms summed in double.
 * MODE_DETERMINISTIC: every row sum in ascending rating index, r_pred serial in f: the factors are bit-identical to the
 * source's single-thread float32 loop (its IEEE semantics, every operation separately rounded).
 * MODE_HOGWILD: rows longer than 256 ratings are summed in pieces of 256 whose partial sums are added in ascending
 * order, r_pred's dot product is a butterfly: exact sums in another, fixed order — the same bits run to run, one owner
 * per accumulator row, no float atomics (a prange build of the reference would race on these +=).
 * The bias pass is sequential-exact in both modes: below 4096 ratings (or after a refused cooperative launch) the level
 * schedule, above one persistent dataflow launch with the users owned and the item bias handed over by version counters.
 * Any k >= 1.  The row sums live in registers up to k = 256 (lane groups of pow2 >= k lanes: 8, 4, 2 rows per wave up
 * to k = 32); beyond that one wave per row keeps them in memory. */
/* float32 U [n_users,k], V [n_items,k]; Bu [n_users], Bi [n_items] may be NULL: zeros (recom_nmf.pyx:134-145) */
int cornac_hip_mf_nmf_set_factors(cornac_hip_mf_t h, const float *U, const float *V, const float *Bu, const float *Bi);
/* any pointer may be NULL */
int cornac_hip_mf_nmf_get_factors(cornac_hip_mf_t h, float *U, float *V, float *Bu, float *Bi);
/* n_epochs epochs of recom_nmf.pyx:217-259; mode: CORNAC_HIP_MODE_*; loss_per_epoch [n_epochs] may be NULL */
int cornac_hip_mf_nmf_fit(cornac_hip_mf_t h, int n_epochs, float lr, float lambda_u, float lambda_v, float lambda_bu,
                          float lambda_bi, float mu, int use_bias, int mode, double *loss_per_epoch);
/* the kernels of the last epoch (0 = none yet): *sum_form 1 ordered / 2 free-order; *bias_form 0 none / 1 dataflow launch /
 * 2 level schedule (the prange body's bias lines, :236-238); *rows_split rows summed in more than one piece */
int cornac_hip_mf_nmf_form(cornac_hip_mf_t h, int *sum_form, int *bias_form, int *rows_split);

/* HPF on the same handle: Poisson factorisation's variational updates in float64, tables of their own (the MF, PMF and NMF
 * state of the handle is untouched, and their fits leave these alone).
 * Replaces: hpf_cpp(tX, k, G_s, G_r, L_s, L_r, K_r, T_r, maxiter)   cornac/models/hpf/cpp/cpp_hpf.cpp:208-275
 *           pf_cpp (the same arguments)                              cornac/models/hpf/cpp/cpp_hpf.cpp:139-203
 *           as hpf.hpf / hpf.pf call them (cornac/models/hpf/cython/hpf.pyx:100-164 / :35-97).
 * The handle's ratings must be stored by user (rid non-decreasing), as for NMF: cornac_hip_mf_hpf_fit refuses any other
 * order.  One iteration (prior = 0.3, eps = 2^-52, k_s = t_s = 0.3 (1 + k) hierarchical / 0.3 otherwise):
 *   Lt = exp(digamma(G_s) - log G_r), Lb = exp(digamma(L_s) - log L_r)                       (cpp_hpf.cpp:102-123, :240-244)
 *   G_s[u,f] = prior + sum over u's ratings of Lt[u,f] Lb[i,f] x / (eps + sum_f Lt[u,f] Lb[i,f])         (cpp_hpf.cpp:41-61)
 *   G_r[u,f] = k_s / K_r[u] + sum_j L_s[j,f] / L_r[j,f], from the L of the iteration before              (cpp_hpf.cpp:22-37)
 *   hierarchical: K_r[u] = 0.3 + sum_f G_s[u,f] / G_r[u,f]                                               (cpp_hpf.cpp:7-19)
 *   L_s, L_r, T_r likewise by item, from the same Lt and Lb and from the new G                           (cpp_hpf.cpp:65-84)
 * Every table must be strictly positive and finite (the caller checks): the reference's detour through pruned sparse
 * matrices is this dense formula then, and its treatment of zeros is not reproduced.
 * One mode.  Every sum takes a fixed order of its own (rows longer than 256 ratings in pieces added in ascending order,
 * the column sums as trees): the same bits run to run, one owner per accumulator row, no float atomics.  The reference's
 * own order cannot be held bit for bit (digamma, log and exp are other implementations); results are compared with a
 * tolerance.  k <= 256: a row's sums live in registers. */
/* float64 G_s, G_r [n_users,k], L_s, L_r [n_items,k], all required; k > 256: CORNAC_HIP_ERR_INVALID */
int cornac_hip_mf_hpf_set_tables(cornac_hip_mf_t h, const double *G_s, const double *G_r, const double *L_s, const double *L_r);
/* any pointer may be NULL; K_r [n_users], T_r [n_items] as the last fit left them */
int cornac_hip_mf_hpf_get_tables(cornac_hip_mf_t h, double *G_s, double *G_r, double *L_s, double *L_r, double *K_r, double *T_r);
/* n_iters iterations of cpp_hpf.cpp:238-273 (hierarchical != 0) or :166-201.  As there, K_r = T_r = 1 at the start of every
 * call (hpf.pyx:148-149) and, hierarchical, are then computed from the tables (cpp_hpf.cpp:231-234): 1 + 2 iterations
 * over two calls give the bits of 3 */
int cornac_hip_mf_hpf_fit(cornac_hip_mf_t h, int n_iters, int hierarchical);
/* the expected-log step alone on the current tables (cpp_hpf.cpp:240-244): Lt [n_users,k], Lb [n_items,k], either may be NULL */
int cornac_hip_mf_hpf_elog(cornac_hip_mf_t h, double *Lt, double *Lb);
/* the last iteration (0 = none yet): *group lanes per row, *rows_split rows summed in more than one piece */
int cornac_hip_mf_hpf_form(cornac_hip_mf_t h, int *group, int *rows_split);

/* Minibatch path with dense optimisers on the same handle.
 * Replaces: backend_pt.learn(model, train_set, n_epochs, batch_size, learning_rate, reg, optimizer)
 *           cornac/models/mf/backend_pt.py:67-106 and the forward of backend_pt.MF (:56-65), selected by
 *           MF(backend="pytorch", optimizer=...) (cornac/models/mf/recom_mf.py:211-252).
 * order: indices into the handle's rating arrays in visiting order (the concatenated batches of
 * Dataset.uir_iter(batch_size, shuffle=True), cornac/data/dataset.py:445-488); consecutive slices of batch_size
 * form the optimiser steps (the last one may be shorter).  Optimiser state persists across calls. */
#define CORNAC_HIP_OPT_SGD 0
#define CORNAC_HIP_OPT_ADAM 1
#define CORNAC_HIP_OPT_RMSPROP 2
#define CORNAC_HIP_OPT_ADAGRAD 3
int cornac_hip_mf_fit_minibatch(cornac_hip_mf_t h, const int64_t *order, int64_t n_total, int batch_size,
                                int optimizer, float lr, float reg, float mu, int use_bias, double *loss_sum);
/* The same with the reference's dropout on the gathered rows (backend_pt.py:42,59: nn.Dropout(p) on the user rows and on
 * the item rows of a batch): keep_u / keep_i are [n_total][k] bytes, row b belongs to order[b], non-zero = the factor is
 * kept and scaled by keep_scale = 1 / (1 - p).  The masks are an input: the host draws them as the reference's run
 * draws them from torch's CPU generator (cornac_amd/mf.py). */
int cornac_hip_mf_fit_minibatch_dropout(cornac_hip_mf_t h, const int64_t *order, int64_t n_total, int batch_size,
                                        int optimizer, float lr, float reg, float mu, int use_bias, const uint8_t *keep_u,
                                        const uint8_t *keep_i, float keep_scale, double *loss_sum);
int cornac_hip_mf_reset_optimizer(cornac_hip_mf_t h);

/* ------------------------------------------------------------------------- *
 * VBPR (visual BPR) minibatch trainer.
 * Replaces: the per-batch body of VBPR._fit_torch (forward, autograd backward,
 *           torch.optim.Adam step over all tables) cornac/models/vbpr/recom_vbpr.py:228-262.
 * The (u, i, j) batches are produced by the host sampler Dataset.uij_iter
 * (cornac/data/dataset.py:490-526) exactly as in the reference and handed over
 * per call; Adam moments and the step counter persist in the handle.
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_vbpr *cornac_hip_vbpr_t;

/* features: item visual features [n_items, n_feat] fp32 (train_set.item_image.features) */
int cornac_hip_vbpr_create(cornac_hip_vbpr_t *out, int device, int64_t n_users, int64_t n_items, int k, int k2,
                           int n_feat, const float *features);
int cornac_hip_vbpr_destroy(cornac_hip_vbpr_t h);
/* Bi [n_items], Gu [n_users,k], Gi [n_items,k], Tu [n_users,k2], E [n_feat,k2], Bp [n_feat]; NULL skips */
int cornac_hip_vbpr_set_params(cornac_hip_vbpr_t h, const float *Bi, const float *Gu, const float *Gi, const float *Tu,
                               const float *E, const float *Bp);
int cornac_hip_vbpr_get_params(cornac_hip_vbpr_t h, float *Bi, float *Gu, float *Gi, float *Tu, float *E, float *Bp);
/* runs ceil(n_total / batch_size) Adam steps over consecutive batches of the triplet arrays;
 * sum_nll (may be NULL) receives sum over all triplets of -logsigmoid(x_uij) */
int cornac_hip_vbpr_fit_batches(cornac_hip_vbpr_t h, const int32_t *u, const int32_t *i, const int32_t *j,
                                int64_t n_total, int batch_size, float lr, float lambda_w, float lambda_b,
                                float lambda_e, double *sum_nll);
/* theta_item = F E [n_items, k2], visual_bias = F Bp [n_items] (recom_vbpr.py:132-133) */
int cornac_hip_vbpr_item_tables(cornac_hip_vbpr_t h, float *theta_item, float *visual_bias);

/* ------------------------------------------------------------------------- *
 * WMF (weighted matrix factorisation) minibatch trainer.
 * Replaces: the TensorFlow graph of cornac/models/wmf/wmf.py:34-55 (P = U V_b^T, weighted
 *           squared error, gradient clipping to [-5, 5], tf.train.AdamOptimizer) and the
 *           per-batch sess.run of cornac/models/wmf/recom_wmf.py:181-199.
 * Batches of item ids come from the host iterator Dataset.item_iter (cornac/data/dataset.py:546-562)
 * exactly as in the reference; Adam moments and the step counter persist in the handle and are
 * reset by set_factors (the reference builds a fresh graph per fit).
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_wmf *cornac_hip_wmf_t;

/* CSC of the rating matrix (train_set.csc_matrix): indptr int64[n_items+1], rows = user ids, vals fp32 */
int cornac_hip_wmf_create(cornac_hip_wmf_t *out, int device, int64_t n_users, int64_t n_items, int k,
                          const int64_t *csc_indptr, const int32_t *csc_rows, const float *csc_vals, int64_t nnz);
void cornac_hip_wmf_destroy(cornac_hip_wmf_t h);
/* U [n_users,k], V [n_items,k] fp32 */
int cornac_hip_wmf_set_factors(cornac_hip_wmf_t h, const float *U, const float *V);
int cornac_hip_wmf_get_factors(cornac_hip_wmf_t h, float *U, float *V);
/* one Adam step per batch b = item_ids[batch_ptr[b] .. batch_ptr[b+1]) (1..128 distinct items), in order;
 * loss_out[b] (may be NULL) = that step's loss value (`_loss`, recom_wmf.py:195).  The whole call is checked before
 * anything is enqueued: an id out of range, an item twice in one batch, a batch of 0 or more than 128 items, or a step
 * count that would reach 2^25 since the last set_factors fails with CORNAC_HIP_ERR_INVALID and changes nothing */
int cornac_hip_wmf_fit_batches(cornac_hip_wmf_t h, const int32_t *item_ids, const int64_t *batch_ptr,
                               int64_t n_batches, float lambda_u, float lambda_v, float a, float b,
                               float learning_rate, double *loss_out);
/* HIP-event timing of fit_batches (device ms of the last call) */
int cornac_hip_wmf_kernel_timing(cornac_hip_wmf_t h, int enabled);
int cornac_hip_wmf_last_timing(cornac_hip_wmf_t h, double *device_ms);

/* ------------------------------------------------------------------------- *
 * Scoring / ranking.
 * Replaces: fast_dot(vec, mat, output)  cornac/utils/fast_dot.pyx:40-43 as used by
 *           BPR.score (recom_bpr.pyx:288-291) and MF.score (recom_mf.py:273-278),
 *           and the per-user argsort/argpartition of Recommender.rank
 *           (cornac/models/recommender.py:503-530), batched over users.
 * score(u, i) = item_base[i] + user_base[u] + sum_f U[u,f]*V[i,f], accumulated
 * as an index-ordered fp32 fma chain (what the gfx950 fp32 MFMA computes).
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_scorer *cornac_hip_scorer_t;

/* Exclusion lists per USER id, kept on the device: CSR (indptr int64[n_users + 1], indices int32) of the items
 * ranking must skip for each user — in the evaluation loop the user's training (+ validation) positives
 * (cornac/eval_methods/base_method.py:176-205 builds the same list per user with numpy set operations).  NULL indptr
 * drops them.  cornac_hip_rank_topk_resident ranks `n` users (users[0..n), or u0 .. u0+n-1 when users is NULL) with
 * those lists applied, like cornac_hip_rank_topk with per-call lists but without moving the lists again; items_out /
 * scores_out may be NULL (results stay on the device), device_ms (optional) receives the HIP-event time of the
 * bitmap build + fused top-k + merge kernels. */
int cornac_hip_scorer_set_exclusions(cornac_hip_scorer_t h, const int64_t *indptr, const int32_t *indices);
/* Page-locked host memory of at least `bytes` bytes owned by the scorer (re-used across calls, freed with it): a caller
 * that passes it as items_out / scores_out gets its results at the full PCIe rate instead of through the pageable-copy
 * staging path (5.5 MB of top-10 ids for 138 493 users: 0.2 instead of 0.5 ms).  A later, larger request returns a new
 * buffer; outgrown ones stay valid (and allocated) until the scorer is destroyed. */
int cornac_hip_scorer_host_buffer(cornac_hip_scorer_t h, size_t bytes, void **out);
int cornac_hip_rank_topk_resident(cornac_hip_scorer_t h, const int32_t *users, int64_t u0, int64_t n, int topk,
                                  int32_t *items_out, float *scores_out, double *device_ms);

int cornac_hip_scorer_create(cornac_hip_scorer_t *out, int device, int64_t n_users, int64_t n_items, int k);
int cornac_hip_scorer_destroy(cornac_hip_scorer_t h);
/* item_base: BPR -> i_biases; MF -> global_mean + i_biases.  user_base: MF -> u_biases; NULL = 0. */
int cornac_hip_scorer_set(cornac_hip_scorer_t h, const float *U, const float *V, const float *item_base,
                          const float *user_base);
/* out[n_items] for one user  (= model.score(user_idx)) */
int cornac_hip_score_user(cornac_hip_scorer_t h, int64_t user, float *out);
/* fast_dot's float64 variant (cornac/utils/fast_dot.pyx:25-43, ddot): the scorer can additionally hold the float64 tables
 * of a model trained in double; score_user_f64 = item_base + user_base + <U[user], V[i]> summed in index order in double.
 * The batched top-k kernels stay float32 (MFMA): a float64 model ranks through score_user_f64 + the reference's own
 * host-side ordering (cornac/models/recommender.py:503-530 is NumPy). */
int cornac_hip_scorer_set_f64(cornac_hip_scorer_t h, const double *U, const double *V, const double *item_base,
                              const double *user_base);
int cornac_hip_score_user_f64(cornac_hip_scorer_t h, int64_t user, double *out);
/* out[n * n_items] for a block of users */
int cornac_hip_score_block(cornac_hip_scorer_t h, const int32_t *users, int64_t n, float *out);
/* out[p] = score(users[p], items[p]) for n pairs, optionally clipped to [lo, hi]:
 * the batched form of Recommender.rate() (cornac/models/recommender.py:447-474) as
 * called once per test rating by rating_eval (cornac/eval_methods/base_method.py:35-105). */
int cornac_hip_score_pairs(cornac_hip_scorer_t h, const int32_t *users, const int32_t *items, int64_t n, int clip,
                           float lo, float hi, float *out);
/* Batched rank(): for each of the n users, the topk best items in descending
 * score order (ties: higher item index first — the oracle's pinned tie rule),
 * excluding the items listed in the optional CSR (excl_indptr[n+1],
 * excl_indices) row of that user.  topk == n_items gives the full ranking.
 * items_out / scores_out are [n, topk]; slots beyond the number of candidates
 * are filled with -1 / -inf. */
int cornac_hip_rank_topk(cornac_hip_scorer_t h, const int32_t *users, int64_t n, int topk, const int64_t *excl_indptr,
                         const int32_t *excl_indices, int32_t *items_out, float *scores_out);
/* Where listed items stand in each user's ranking, without producing the ranking: for user users[b] the
 * "targets" tgt_indices[tgt_indptr[b] .. tgt_indptr[b+1]) (the evaluation loop's test positives,
 * cornac/eval_methods/base_method.py:185-206) among that user's candidates (all items minus the optional
 * exclusion CSR row, as in cornac_hip_rank_topk).  Per target, in tgt_indices order:
 *   greater_out = candidates with a strictly higher score,
 *   pos_out     = its 0-based position in the order cornac_hip_rank_topk produces (ties: higher index first),
 *   ge_out      = candidates with score >= its own (itself included),
 *   tgt_scores_out = its score.
 * These are what AUC / MAP / MRR (cornac/metrics/ranking.py:185-527) read off `rank(k=-1)` output.  A target that is
 * out of range or excluded gets -1 / -1 / -1 / -inf. */
int cornac_hip_rank_positions(cornac_hip_scorer_t h, const int32_t *users, int64_t n, const int64_t *excl_indptr,
                              const int32_t *excl_indices, const int64_t *tgt_indptr, const int32_t *tgt_indices,
                              int32_t *greater_out, int32_t *pos_out, int32_t *ge_out, float *tgt_scores_out);
/* Device-resident throughput probe used by bench.py: ranks users
 * [u0, u0 + n) with fused top-k, keeps results on device; returns elapsed ms of
 * the kernels (hipEvent) in *ms. */
int cornac_hip_rank_topk_device(cornac_hip_scorer_t h, int64_t u0, int64_t n, int topk, int repeats, double *ms);

/* ------------------------------------------------------------------------- *
 * Neighbourhood models (UserKNN / ItemKNN), float64 throughout.
 * Replaces: compute_similarity, compute_score and compute_score_single of
 *           cornac/models/knn/similarity.pyx:51-201 with the TopK / SparseNeighbors
 *           helpers of cornac/models/knn/similarity.h, as called by
 *           cornac/models/knn/recom_knn.py:205, :240-261, :382, :413-434.
 * Every CSR here has sorted column indices without repeats (checked).
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_knn_sim *cornac_hip_knn_sim_t;
typedef struct cornac_hip_knn_scorer *cornac_hip_knn_scorer_t;
/* largest neighbourhood size k of the scoring calls */
#define CORNAC_HIP_KNN_MAX_K 64

/* compute_similarity(data_mat) (similarity.pyx:51-105; its k argument is unused there): W is the CSR
 * [n_rows x n_cols] of data_mat.  For every row r and every row i sharing a column with it,
 * S[r,i] = sum x*w over the shared columns in r's stored order, divided (where it is != 0) by sqrt(d1 * d2) with d1 / d2
 * the sums of w*w / x*x over the shared columns whose two values are both != 0 -- the quotient of the extension as the
 * reference compiles it (-ffast-math, setup.py:128-138).  The result holds exactly the entries that are != 0, ascending
 * column indices, the diagonal included. */
int cornac_hip_knn_sim_create(cornac_hip_knn_sim_t *out, int device, int64_t n_rows, int64_t n_cols, const int64_t *indptr,
                              const int32_t *indices, const double *data);
int cornac_hip_knn_sim_destroy(cornac_hip_knn_sim_t h);
/* rows_per_pass rows at a time, each with three accumulators of n_rows doubles in device scratch (the reference's
 * per-thread denom1 / denom2 and its dense sim_mat row, similarity.pyx:66-74); 0 = as many as half of the free device
 * memory holds.  The result does not depend on it, and a repeated run gives the same bits.  Fails with
 * CORNAC_HIP_ERR_HIP and a message naming the buffer when the scratch or the result cannot be allocated. */
int cornac_hip_knn_sim_run(cornac_hip_knn_sim_t h, int64_t rows_per_pass);
/* entries of the result of the last run, then the result itself: indptr[n_rows + 1], indices[nnz], data[nnz]
 * (csr_matrix(sim_mat), similarity.pyx:102) */
int cornac_hip_knn_sim_nnz(cornac_hip_knn_sim_t h, int64_t *nnz);
int cornac_hip_knn_sim_get(cornac_hip_knn_sim_t h, int64_t *indptr, int32_t *indices, double *data);

/* compute_score / compute_score_single (similarity.pyx:108-201).  N: the neighbour table, CSR [n_items x n_neighbours]
 * (UserKNN: iu_mat; ItemKNN: sim_mat); Q: CSR [n_users x n_neighbours] whose row u, made dense, is the call's sim_arr
 * (UserKNN: sim_mat; ItemKNN: ui_mat).  The candidates of item i are the entries (nn, s) of N's row i with
 * Q[u, nn] != 0 (a stored zero is no candidate); (weight, rating) = (Q[u,nn], s) if user_mode, else (s, Q[u,nn]).  The
 * survivors are those of the reference's heap of k pairs fed in reverse stored order (similarity.h:15-38, :62-79), ties
 * at the k-th weight included; out = sum w*s / (sum |w| + 1e-8) over them, 0 without candidates.  1 <= k <=
 * CORNAC_HIP_KNN_MAX_K.  Weights must not be NaN. */
int cornac_hip_knn_scorer_create(cornac_hip_knn_scorer_t *out, int device, int64_t n_items, int64_t n_neighbours,
                                 int64_t n_users, const int64_t *n_indptr, const int32_t *n_indices, const double *n_data,
                                 const int64_t *q_indptr, const int32_t *q_indices, const double *q_data, int user_mode);
int cornac_hip_knn_scorer_destroy(cornac_hip_knn_scorer_t h);
/* out[n x n_items]: compute_score for each listed user (similarity.pyx:154-201) */
int cornac_hip_knn_scorer_score_users(cornac_hip_knn_scorer_t h, const int32_t *users, int64_t n, int k, double *out);
/* out[n]: compute_score_single for each (users[p], items[p]) (similarity.pyx:109-150); the bits of the matching
 * score_users entry */
int cornac_hip_knn_scorer_score_pairs(cornac_hip_knn_scorer_t h, const int32_t *users, const int32_t *items, int64_t n, int k,
                                      double *out);

/* ------------------------------------------------------------------------- *
 * EASE (Steck 2019), float64 throughout.
 * Replaces: the NumPy / SciPy body of EASE.fit and EASE.score,
 *           cornac/models/ease/recom_ease.py:72-97 and :123-126.
 * The handle owns X = train_set.matrix on the device (CSR as given, sorted indices without repeats, finite values --
 * all checked -- and its CSC) and ONE dense [n_items x n_items] row-major table, which is G, then P, then B, in place.
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_ease *cornac_hip_ease_t;

/* Fails with CORNAC_HIP_ERR_HIP and a message stating the bytes wanted when the table cannot be allocated.  The table
 * starts as zeros. */
int cornac_hip_ease_create(cornac_hip_ease_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, const double *data);
int cornac_hip_ease_destroy(cornac_hip_ease_t h);
/* table <- X^T X (recom_ease.py:78): G[i, j] = sum over the users in ascending order of x_ui * x_uj, product and sum rounded
 * separately -- the bits of SciPy's sparse product.  A repeated run gives the same bits. */
int cornac_hip_ease_gram(cornac_hip_ease_t h);
/* table <- inv(table + lamb I) (recom_ease.py:80-84) by blocked Gauss-Jordan without pivoting, block 64, every sum in
 * one fixed order.  lamb must be > 0 (a departure from the reference, which hands a singular G to NumPy).  A pivot that
 * is not a positive finite number makes the call return CORNAC_HIP_ERR_INVALID with "... not positive definite at block
 * N" once the sweep is through; the table then holds no inverse, and the handle stays usable. */
int cornac_hip_ease_invert(cornac_hip_ease_t h, double lamb);
/* table <- B (recom_ease.py:86-92): column j divided by -P_jj, the diagonal 0, and with pos_b every entry that is not
 * above 0 replaced by +0.0 */
int cornac_hip_ease_weights(cornac_hip_ease_t h, int pos_b);
/* gram, invert, weights in one call: the same bits as the three calls */
int cornac_hip_ease_fit(cornac_hip_ease_t h, double lamb, int pos_b);
/* the table to / from table[n_items * n_items] on the host */
int cornac_hip_ease_get_table(cornac_hip_ease_t h, double *table);
int cornac_hip_ease_set_table(cornac_hip_ease_t h, const double *table);
/* out[n x n_items] = X[users[b], :] . table (recom_ease.py:124): y = 0, then y += x * table[j, :] over the user's entries in
 * ascending item order, product and sum rounded separately -- the bits of SciPy's csr . dense */
int cornac_hip_ease_score_users(cornac_hip_ease_t h, const int32_t *users, int64_t n, double *out);
/* out[n]: X[users[p], :] . table[:, items[p]] (recom_ease.py:126); the bits of the matching score_users entry */
int cornac_hip_ease_score_pairs(cornac_hip_ease_t h, const int32_t *users, const int32_t *items, int64_t n, double *out);

/* ------------------------------------------------------------------------- *
 * VAECF (Liang et al. 2018, "Mult-VAE"), float32 throughout, one hidden layer.
 * Replaces: VAE.forward / VAE.loss / learn, cornac/models/vaecf/vaecf.py:37-149, and VAECF.score,
 *           cornac/models/vaecf/recom_vaecf.py:193-202.
 * The handle owns the binarised training CSR (sorted indices without repeats, checked; stored values are never read:
 * every stored entry counts as 1, as `u_batch.data = ones` does at vaecf.py:131), its CSC, the ten tables with Adam's m
 * and v, and Adam's step counter t, which persist across calls.  Tables are passed as arrays of ten pointers in the order
 * and with the shapes of the reference's state_dict:
 *   0 encoder.fc0.weight [h x I]   1 encoder.fc0.bias [h]   2 enc_mu.weight [k x h]      3 enc_mu.bias [k]
 *   4 enc_logvar.weight [k x h]    5 enc_logvar.bias [k]    6 decoder.fc0.weight [h x k] 7 decoder.fc0.bias [h]
 *   8 decoder.fc1.weight [I x h]   9 decoder.fc1.bias [I]
 * (the device keeps table 0 transposed).  A NULL entry skips its table.
 * act: 0 tanh, 1 sigmoid, 2 relu, 3 relu6, 4 elu (alpha 1).  likelihood: 0 mult, 1 bern, 2 gaus, 3 pois.
 * Supported: 1 <= k <= 256, 1 <= h <= 1024, 1 <= batch_size <= 1024; anything else is CORNAC_HIP_ERR_INVALID with a
 * message naming the limit.  No float atomics; every sum has one fixed order: the same inputs give the same bits.
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_vaecf *cornac_hip_vaecf_t;

/* vaecf.py:38-64 (the model's shape) and :130-133 (the batch rows, here never densified); all tables start as zeros */
int cornac_hip_vaecf_create(cornac_hip_vaecf_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                            const int32_t *indices, int k, int h, int act, int likelihood);
int cornac_hip_vaecf_destroy(cornac_hip_vaecf_t h);
/* the ten tables from / to the host (state_dict of vaecf.py:37-64) */
int cornac_hip_vaecf_set_params(cornac_hip_vaecf_t h, const float *const *tables);
int cornac_hip_vaecf_get_params(cornac_hip_vaecf_t h, float *const *tables);
/* Adam's exp_avg (m) and exp_avg_sq (v), in the tables' shapes, and its step counter (vaecf.py:120); NULL skips */
int cornac_hip_vaecf_get_state(cornac_hip_vaecf_t h, float *const *m, float *const *v, int64_t *t);
/* m = v = 0, t = 0: what a new torch.optim.Adam (vaecf.py:120, once per learn()) starts from */
int cornac_hip_vaecf_reset_optimizer(cornac_hip_vaecf_t h);
/* One epoch of vaecf.py:127-144: ceil(n_users / batch_size) steps over consecutive user ranges (user_iter without
 * shuffling), each a forward, a backward and torch.optim.Adam's dense sweep (betas 0.9 / 0.999, eps 1e-8) over every
 * table, enqueued from this one call with one synchronise at the end.  eps [n_users x k] is the noise of
 * reparameterize() (vaecf.py:79), row = user; NULL draws it on the device (Philox keyed by seed, step, user, factor).
 * loss_sum: the sum over the steps of the batch-mean loss (`sum_loss` of vaecf.py:143); step_loss [steps]: each of them.
 * Either may be NULL. */
int cornac_hip_vaecf_fit_epoch(cornac_hip_vaecf_t h, int64_t batch_size, float lr, float beta, const float *eps, uint64_t seed,
                               double *loss_sum, double *step_loss);
/* h2_out [n x h]: the decoder's hidden layer at z = mu(x_u) (recom_vaecf.py:194-196 and the first half of decode):
 * score = softmax / sigmoid of c1 + <h2(u), D1[i]>, so (h2, D1, c1) are a factor model's ranking tables */
int cornac_hip_vaecf_encode_users(cornac_hip_vaecf_t h, const int32_t *users, int64_t n, float *h2_out);
/* out [n x n_items] = decode(mu(x_u)) (recom_vaecf.py:193-197); score_pairs: out[p] is the entry items[p] of users[p]'s
 * row (recom_vaecf.py:198-202), the bits of the matching score_users entry */
int cornac_hip_vaecf_score_users(cornac_hip_vaecf_t h, const int32_t *users, int64_t n, float *out);
int cornac_hip_vaecf_score_pairs(cornac_hip_vaecf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out);

/* ------------------------------------------------------------------------- *
 * BiVAECF (Truong, Salah, Lauw 2021, "Bilateral VAE"), float32 throughout, one hidden layer per encoder, standard normal
 * priors (no CAP priors).
 * Replaces: BiVAE.forward / BiVAE.loss / learn, cornac/models/bivaecf/bivae.py:34-276, and BiVAECF.score,
 *           cornac/models/bivaecf/recom_bivaecf.py:193-225.
 * The handle owns the binarised training CSR (sorted indices without repeats, checked; stored values are never read:
 * every stored entry counts as 1, as bivae.py:190 does), its CSC, the 12 tables with Adam's m and v, one Adam step counter
 * per side, and the four factor tables theta [U x k], beta [I x k], mu_theta [U x k], mu_beta [I x k] (bivae.py:48-53),
 * all of which persist across calls.  Tables are passed as arrays of 12 pointers in the order and with the shapes of the
 * reference's state_dict:
 *   0 user_encoder.fc0.weight [h x I]   1 user_encoder.fc0.bias [h]   2 user_mu.weight [k x h]    3 user_mu.bias [k]
 *   4 user_std.weight [k x h]           5 user_std.bias [k]
 *   6 item_encoder.fc0.weight [h x U]   7 item_encoder.fc0.bias [h]   8 item_mu.weight [k x h]    9 item_mu.bias [k]
 *  10 item_std.weight [k x h]          11 item_std.bias [k]
 * (the device keeps tables 0 and 6 transposed).  A NULL entry skips its table.
 * act: 0 tanh, 1 sigmoid, 2 relu, 3 relu6, 4 elu (alpha 1).  likelihood: 0 bern, 1 gaus, 2 pois.
 * Supported: 1 <= k <= 256, 1 <= h <= 1024, 1 <= batch_size <= 1024; anything else is CORNAC_HIP_ERR_INVALID with a
 * message naming the limit.  No float atomics; every sum has one fixed order: the same inputs give the same bits.
 * The decoder's B x N probabilities (bivae.py:111-117) are never stored: a fused pass over fixed ranges of
 * CORNAC_HIP_BIVAE_RANGE rows of the other side's table gives each batch row's log-likelihood and gradient.
 * ------------------------------------------------------------------------- */
#define CORNAC_HIP_BIVAE_RANGE 512
typedef struct cornac_hip_bivae *cornac_hip_bivae_t;

/* bivae.py:35-86 (the model's shape) and :189-191 (X and its transpose, here never densified); all tables start as zeros */
int cornac_hip_bivae_create(cornac_hip_bivae_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                            const int32_t *indices, int k, int h, int act, int likelihood);
int cornac_hip_bivae_destroy(cornac_hip_bivae_t h);
/* the 12 tables from / to the host (state_dict of bivae.py:66-86) */
int cornac_hip_bivae_set_params(cornac_hip_bivae_t h, const float *const *tables);
int cornac_hip_bivae_get_params(cornac_hip_bivae_t h, float *const *tables);
/* theta, beta, mu_theta, mu_beta (bivae.py:48-53) from / to the host; NULL skips */
int cornac_hip_bivae_set_factors(cornac_hip_bivae_t h, const float *theta, const float *beta, const float *mu_theta,
                                 const float *mu_beta);
int cornac_hip_bivae_get_factors(cornac_hip_bivae_t h, float *theta, float *beta, float *mu_theta, float *mu_beta);
/* Adam's exp_avg (m) and exp_avg_sq (v), in the tables' shapes, and the step counters of u_optimizer and i_optimizer
 * (bivae.py:186-187); NULL skips */
int cornac_hip_bivae_get_state(cornac_hip_bivae_t h, float *const *m, float *const *v, int64_t *t_user, int64_t *t_item);
/* m = v = 0, both counters 0: what the two new torch.optim.Adam of bivae.py:186-187 (once per learn()) start from */
int cornac_hip_bivae_reset_optimizer(cornac_hip_bivae_t h);
/* One epoch of bivae.py:194-256: ceil(n_items / batch_size) item steps, then ceil(n_users / batch_size) user steps, over
 * consecutive id ranges (item_iter / user_iter without shuffling).  A step is a forward against the other side's whole
 * sampled table as it stands (a constant), the backward, torch.optim.Adam's dense sweep (betas 0.9 / 0.999, eps 1e-8)
 * over the side's six tables, and a second forward with the updated tables whose sample and mean go to the side's rows
 * of beta / mu_beta or theta / mu_theta (bivae.py:220-223, 250-252).  All of it is enqueued from this one call with one
 * synchronise at the end.  eps_item [2 x n_items x k], eps_user [2 x n_users x k]: plane 0 is the noise of the training
 * forward's reparameterize() (bivae.py:119-121), plane 1 that of the forward after the step, row = id; NULL draws on the
 * device (Philox keyed by seed, side, step, draw, row, factor).  loss_item / loss_user: the sum over the side's steps of
 * the batch-mean loss (i_sum_loss / u_sum_loss of bivae.py:217, 247); step_loss [item steps + user steps]: each of them,
 * item steps first.  Any may be NULL. */
int cornac_hip_bivae_fit_epoch(cornac_hip_bivae_t h, int64_t batch_size, float lr, float beta_kl, const float *eps_item,
                               const float *eps_user, uint64_t seed, double *loss_item, double *loss_user, double *step_loss);
/* device time (stream events) of the last fit_epoch's item pass and user pass, noise upload or generation included, in
 * milliseconds; either may be NULL */
int cornac_hip_bivae_last_timing(cornac_hip_bivae_t h, double *item_ms, double *user_ms);
/* bivae.py:258-274: mu_beta and mu_theta again from the tables as they stand */
int cornac_hip_bivae_infer_means(cornac_hip_bivae_t h);
/* out [n x n_items] = sigmoid(mu_theta[u] . mu_beta^T) (recom_bivaecf.py:217-220); score_pairs: out[p] is the entry
 * items[p] of users[p]'s row (recom_bivaecf.py:221-224, before its scaling), the bits of the matching score_users entry.
 * An id out of range is named in the error. */
int cornac_hip_bivae_score_users(cornac_hip_bivae_t h, const int32_t *users, int64_t n, float *out);
int cornac_hip_bivae_score_pairs(cornac_hip_bivae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out);

/* ------------------------------------------------------------------------------------------------
 * Neural collaborative filtering (He et al. 2017): GMF, MLP and NeuMF, float32 throughout, the PyTorch backend's semantics.
 * Replaces: GMF / MLP / NeuMF .forward, cornac/models/ncf/backend_pt.py:22-175; the batch loop of _fit_pt,
 *           cornac/models/ncf/recom_ncf_base.py:240-293 (one step: :266-281); the sampler it calls,
 *           Dataset.uir_iter(num_zeros=), cornac/data/dataset.py:445-488; and _score_pt,
 *           cornac/models/ncf/recom_gmf.py:162-173, recom_mlp.py:172-183, recom_neumf.py:277-291.
 * One handle holds the training CSR with its values, the model's tables in the reference's state_dict order and shapes
 *   GMF    user_embedding.weight [U x F], item_embedding.weight [I x F], logit.weight [1 x F], logit.bias [1]
 *   MLP    user_embedding.weight [U x L0/2], item_embedding.weight [I x L0/2], mlp_model.{0,2,..}.weight [L(l+1) x L(l)] and
 *          .bias, logit.weight [1 x L(-1)], logit.bias
 *   NeuMF  logit.weight [1 x (F + L(-1))], logit.bias, gmf.<GMF's four>, mlp.<MLP's>
 * two state arrays per table for the learner, and one step counter.  NeuMF's gmf.logit.* and mlp.logit.* take no part in
 * forward() and have no gradient: no learner touches them or their state (torch skips parameters whose grad is None).
 * Limits, each a named refusal: 1 <= num_factors <= 256; 2 <= n_layers <= 8; layers[0] even in 2 .. 512; every other width
 * in 1 .. 256; 1 <= samples of a step <= 16384; NeuMF needs layers[n_layers - 1] == num_factors (backend_pt.py:139).
 * No float atomics; every sum has one fixed order; the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cornac_hip_ncf *cornac_hip_ncf_t;
enum { CORNAC_HIP_NCF_GMF = 0, CORNAC_HIP_NCF_MLP = 1, CORNAC_HIP_NCF_NEUMF = 2 };
enum { CORNAC_HIP_NCF_ADAM = 0, CORNAC_HIP_NCF_SGD = 1, CORNAC_HIP_NCF_RMSPROP = 2, CORNAC_HIP_NCF_ADAGRAD = 3 };

/* backend_pt.py:22-37, 61-85, 122-147.  indptr / indices / data: the training CSR with sorted indices and finite values (the
 * sampler's `dok_matrix[u, j] > 0`).  num_factors is ignored for MLP, layers / act for GMF.  act: 0 sigmoid, 1 tanh, 2 elu,
 * 3 selu, 4 relu, 5 relu6, 6 leaky_relu (slope 0.01), backend_pt.py:11-19.  All tables start as zeros. */
int cornac_hip_ncf_create(cornac_hip_ncf_t *out, int device, int kind, int64_t n_users, int64_t n_items, const int64_t *indptr,
                          const int32_t *indices, const double *data, int num_factors, const int *layers, int n_layers, int act);
int cornac_hip_ncf_destroy(cornac_hip_ncf_t h);
/* the number of tables: 4 (GMF), 4 + 2 (n_layers - 1) (MLP), their sum + 2 (NeuMF) */
int cornac_hip_ncf_n_tables(cornac_hip_ncf_t h, int *n);
/* the tables from / to the host, in state_dict order; a NULL entry is skipped */
int cornac_hip_ncf_set_params(cornac_hip_ncf_t h, const float *const *tables);
int cornac_hip_ncf_get_params(cornac_hip_ncf_t h, float *const *tables);
/* the learner's state in the tables' shapes and its step counter: adam s1 = exp_avg, s2 = exp_avg_sq; rmsprop s1 = square_avg;
 * adagrad s1 = sum; otherwise zeros.  NULL skips. */
int cornac_hip_ncf_get_state(cornac_hip_ncf_t h, float *const *s1, float *const *s2, int64_t *t);
/* state = 0, t = 0: what the new optimiser of recom_ncf_base.py:255-259 (once per fit) starts from */
int cornac_hip_ncf_reset_optimizer(cornac_hip_ncf_t h);
/* One epoch of recom_ncf_base.py:266-281 over the given samples: step s is the samples [step_ptr[s], step_ptr[s + 1]) of
 * users / items / labels (labels in [0, 1]).  A step: forward, nn.BCELoss (mean; logs clamped at -100), the backward as
 * torch computes it (dL/dp = (p - y) / max(p (1 - p), 1e-12) / n), and the learner's DENSE update of every entry of every
 * table that has a gradient, with g += reg * p first (torch's weight_decay): adam (betas 0.9 / 0.999, eps 1e-8), sgd,
 * rmsprop (alpha 0.99, eps 1e-8), adagrad (eps 1e-10).  The samples are uploaded once and all steps are enqueued from this
 * call, with one synchronise at the end.  loss_sum: the sum of the steps' mean losses; step_loss [steps]: each. */
int cornac_hip_ncf_fit_epoch(cornac_hip_ncf_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users, const int32_t *items,
                             const float *labels, float lr, float reg, int learner, double *loss_sum, double *step_loss);
/* The device sampler's epoch (dataset.py:445-488 in distribution, not draw for draw): the stored entries once each in an order
 * permuted under (seed, epoch), label 1, in steps of batch_size; each step is [positives | negatives, user-major], every
 * positive followed by num_neg items uniform among those j for which (u, j) is not stored with a value > 0, label 0.
 * step_ptr [ceil(nnz / batch_size) + 1]; users, items, labels [nnz * (1 + num_neg)].  Refused by name when num_neg > 0 and
 * some user rates every item positively. */
int cornac_hip_ncf_draw_epoch(cornac_hip_ncf_t h, int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch, int64_t *step_ptr,
                              int32_t *users, int32_t *items, float *labels);
/* fit_epoch over exactly draw_epoch's samples, which never leave the device; step_loss [ceil(nnz / batch_size)] */
int cornac_hip_ncf_fit_epoch_sampled(cornac_hip_ncf_t h, int64_t batch_size, int num_neg, uint64_t seed, uint64_t epoch, float lr,
                                     float reg, int learner, double *loss_sum, double *step_loss);
/* out [n x n_items] = forward(u, every item); score_pairs: out[p] = forward(users[p], items[p]), the bits of the matching
 * score_users entry.  An id out of range is named in the error. */
int cornac_hip_ncf_score_users(cornac_hip_ncf_t h, const int32_t *users, int64_t n, float *out);
int cornac_hip_ncf_score_pairs(cornac_hip_ncf_t h, const int32_t *users, const int32_t *items, int64_t n, float *out);

/* ------------------------------------------------------------------------------------------------
 * LightGCN (He et al. 2020): graph propagation, the BPR step and Adam, float32 throughout.
 * Replaces: construct_graph and its edge norms, cornac/models/lightgcn/lightgcn.py:13-41; GCNLayer.forward and
 *           Model.forward over the whole graph, lightgcn.py:44-117 (DGL's multi_update_all, once per layer, forward and
 *           backward); Model.loss_fn, lightgcn.py:119-134; the batch loop of LightGCN.fit with torch.optim.Adam,
 *           cornac/models/lightgcn/recom_lightgcn.py:143-181 (one step: :168-179); the eval-mode model(graph) of :185-189.
 * One handle holds the normalised adjacency of the bipartite graph as one CSR over the n_users + n_items nodes (the train
 * matrix's rows, then its transpose's, with one float32 weight per edge, (deg_u deg_i)^-1/2 as lightgcn.py:31-39 computes it),
 * the layer-0 tables E0_user [n_users x emb_size] and E0_item [n_items x emb_size], Adam's exp_avg and exp_avg_sq and its
 * step counter.  Nodes without edges are legal.  The final embeddings are E = P(E0), P = 1 / (L + 1) sum_k A^k; P is linear
 * and symmetric, so the gradient of the layer-0 tables is P(G) for the gradient G at the final embeddings: one kernel both
 * ways, no activations kept.
 * Limits, each a named refusal: 1 <= emb_size <= 256; 0 <= num_layers <= 8; 1 <= triplets of a step <= 16384; sorted
 * indices without repeats; nnz < 2^31; n_users + n_items < 2^31.
 * No atomics; every sum has one fixed order (a row's edges ascending, rows longer than 512 edges in pieces combined in
 * piece order, a node's gradient rows in sample order); the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cornac_hip_lightgcn *cornac_hip_lightgcn_t;

/* lightgcn.py:13-41, 64-82.  indptr / indices: the train matrix as a CSR over n_users x n_items (total_users x total_items:
 * rows and columns without entries are nodes without edges).  All tables start as zeros. */
int cornac_hip_lightgcn_create(cornac_hip_lightgcn_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                               const int32_t *indices, int emb_size, int num_layers);
int cornac_hip_lightgcn_destroy(cornac_hip_lightgcn_t h);
/* the layer-0 tables (feature_dict.user, feature_dict.item) from / to the host; NULL skips */
int cornac_hip_lightgcn_set_params(cornac_hip_lightgcn_t h, const float *user, const float *item);
int cornac_hip_lightgcn_get_params(cornac_hip_lightgcn_t h, float *user, float *item);
/* Adam's exp_avg (m) and exp_avg_sq (v) in the tables' shapes and its step counter; NULL skips */
int cornac_hip_lightgcn_get_state(cornac_hip_lightgcn_t h, float *m_user, float *m_item, float *v_user, float *v_item, int64_t *t);
/* state = 0, t = 0: the new torch.optim.Adam of recom_lightgcn.py:143 */
int cornac_hip_lightgcn_reset_optimizer(cornac_hip_lightgcn_t h);
/* One epoch of recom_lightgcn.py:157-179 over the given triplets: step s is [step_ptr[s], step_ptr[s + 1]) of users / pos /
 * neg.  A step of B triplets: E = P(E0); x = <a, n> - <a, p> over the rows a = E_user[u], p = E_item[i], n = E_item[j];
 * bpr = mean softplus(x) (linear above 20), reg = (|a|^2 + |p|^2 + |n|^2) / 2 / B, loss = bpr + lambda_reg reg; the gradient
 * rows (s (n - p) + lambda a) / B, (-s a + lambda p) / B, (s a + lambda n) / B with s = sigmoid(x), summed per node in sample
 * order (an item's positives before its negatives); g = P(G); torch's Adam over every entry of both tables (betas 0.9 /
 * 0.999, eps 1e-8, no weight decay).  The triplets are uploaded once and all steps are enqueued from this call, with one
 * synchronise at the end.  loss_out / bpr_out / reg_out [steps]: each step's three losses; NULL skips. */
int cornac_hip_lightgcn_fit_epoch(cornac_hip_lightgcn_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users,
                                  const int32_t *pos, const int32_t *neg, float lr, float lambda_reg, double *loss_out,
                                  double *bpr_out, double *reg_out);
/* the final embeddings E = P(E0): model(graph) in eval mode, lightgcn.py:92-117 with users = None; NULL skips */
int cornac_hip_lightgcn_propagate(cornac_hip_lightgcn_t h, float *user_out, float *item_out);

/* ------------------------------------------------------------------------------------------------
 * NGCF (Wang et al. 2019): neural graph collaborative filtering, float32 throughout.
 * Replaces: construct_graph, cornac/models/ngcf/ngcf.py:14-37; the edge norms, ngcf.py:110-117; NGCFLayer.forward,
 *           ngcf.py:65-100 (two Linears per edge, DGL's multi_update_all, LeakyReLU, dropout, F.normalize) and
 *           Model.forward over the whole graph, ngcf.py:150-168, forward and backward; Model.loss_fn, ngcf.py:170-185; the
 *           batch loop of NGCF.fit with torch.optim.Adam, cornac/models/ngcf/recom_ngcf.py:148-187 (one step: :173-184); the
 *           eval-mode model(graph) of recom_ngcf.py:190-194.
 * One handle holds LightGCN's adjacency A (one CSR over users then items, float32 weights), the rows' weight sums c, the
 * tables feature_dict.user [n_users x emb_size] and feature_dict.item [n_items x emb_size], per layer W1.weight
 * [d_out x d_in], W1.bias [d_out], W2.weight, W2.bias, Adam's exp_avg and exp_avg_sq of each and its step counter.  The self
 * loop and both edge types collapse to dense work per node:
 *     s = A X;  z = (X + s) W1^T + (s * X) W2^T + b1 + c (b1 + b2);  a = dropout_p(leaky_relu(z, 0.2));
 *     X' = a / max(|a|_2 per row, 1e-12);  E = [X_0 | X_1 | .. | X_L], width D = emb_size + sum(layer_sizes).
 * The dropout mask is the device's own: a pure function of (dropout_key, Adam's step, layer, row, column) through
 * Philox4x32-10, stated in csrc/ngcf.hip; a layer with p = 0 draws nothing.
 * Limits, each a named refusal: 1 <= emb_size <= 256 and every layer size; 1 <= num_layers <= 8; 0 <= p < 1; 1 <= triplets
 * of a step <= 16384; sorted indices without repeats; nnz < 2^31; n_users + n_items < 2^31.
 * No atomics; every sum has one fixed order (the weight and bias gradients: chunks of 2048 rows, added in chunk order); the
 * same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cornac_hip_ngcf *cornac_hip_ngcf_t;

/* ngcf.py:14-37, 103-148.  indptr / indices: the train matrix as a CSR over n_users x n_items (total_users x total_items).
 * layer_sizes / dropout_rates [num_layers].  All parameters start as zeros. */
int cornac_hip_ngcf_create(cornac_hip_ngcf_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                           const int32_t *indices, int emb_size, int num_layers, const int32_t *layer_sizes, const float *dropout_rates,
                           uint64_t dropout_key);
int cornac_hip_ngcf_destroy(cornac_hip_ngcf_t h);
/* the tables and layers [4 num_layers] = per layer W1.weight, W1.bias, W2.weight, W2.bias (ngcf.py:47-48, 141-148) from / to
 * the host; a NULL pointer, a NULL entry and a NULL array skip */
int cornac_hip_ngcf_set_params(cornac_hip_ngcf_t h, const float *user, const float *item, const float *const *layers);
int cornac_hip_ngcf_get_params(cornac_hip_ngcf_t h, float *user, float *item, float *const *layers);
/* Adam's exp_avg (m) and exp_avg_sq (v) in the parameters' shapes and its step counter; NULL skips */
int cornac_hip_ngcf_get_state(cornac_hip_ngcf_t h, float *m_user, float *m_item, float *const *m_layers, float *v_user, float *v_item,
                              float *const *v_layers, int64_t *t);
/* state = 0, t = 0: the new torch.optim.Adam of recom_ngcf.py:148 */
int cornac_hip_ngcf_reset_optimizer(cornac_hip_ngcf_t h);
/* One epoch of recom_ngcf.py:159-184 over the given triplets, in train mode: step s is [step_ptr[s], step_ptr[s + 1]) of
 * users / pos / neg.  The loss is LightGCN's over the rows of E (ngcf.py:170-185); the backward pass is written out in
 * csrc/ngcf.hip; torch's Adam (betas 0.9 / 0.999, eps 1e-8) over every parameter.  The triplets are uploaded once and all
 * steps are enqueued from this call, with one synchronise at the end.  loss_out / bpr_out / reg_out [steps]; NULL skips. */
int cornac_hip_ngcf_fit_epoch(cornac_hip_ngcf_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users, const int32_t *pos,
                              const int32_t *neg, float lr, float lambda_reg, double *loss_out, double *bpr_out, double *reg_out);
/* the concatenated embeddings U [n_users x D], V [n_items x D]: model(graph) in eval mode (no dropout), ngcf.py:150-168 with
 * users = None; NULL skips */
int cornac_hip_ngcf_propagate(cornac_hip_ngcf_t h, float *user_out, float *item_out);

/* ------------------------------------------------------------------------- *
 * RecVAE (Shenbin et al. 2020), float32 throughout.
 * Replaces: Encoder / CompositePrior / VAE.forward / update_prior, cornac/models/recvae/recvae.py:9-117, RecVAE.run,
 *           cornac/models/recvae/recom_recvae.py:127-146, and RecVAE.score, recom_recvae.py:241-278.
 * The handle owns the training CSR with its real values (sorted indices without repeats, finite values, checked; a stored
 * 0.0 contributes nothing), the rows' L2 norms and sums (recvae.py:67, 100), the tables, Adam's m and v of the 26 trainable
 * ones and the two step counters, which persist across calls.  Tables are passed as arrays of 53 pointers in the order and
 * with the shapes of the reference's state_dict (h = hidden_dim, k = latent_dim, I = n_items):
 *    0 .. 23  encoder.:  fc{l}.weight [h x h] (fc1: [h x I]), fc{l}.bias [h], ln{l}.weight [h], ln{l}.bias [h] for l = 1 .. 5,
 *             then fc_mu.weight [k x h], fc_mu.bias [k], fc_logvar.weight [k x h], fc_logvar.bias [k]
 *   24 .. 26  prior.mu_prior, prior.logvar_prior, prior.logvar_uniform_prior [1 x k]
 *   27 .. 50  prior.encoder_old.: as 0 .. 23
 *   51, 52    decoder.weight [I x k], decoder.bias [I]
 * (the device keeps the two fc1.weight tables transposed).  A NULL entry skips its table.  The moments travel as arrays
 * of 26 pointers: the encoder's 24, then the decoder's 2.
 * Supported: 1 <= hidden_dim <= 1024, 1 <= latent_dim <= 256, 1 <= batch_size <= 1024; anything else is
 * CORNAC_HIP_ERR_INVALID with a message naming the limit.  No float atomics; every sum has one fixed order: the same inputs
 * give the same bits.
 * ------------------------------------------------------------------------- */
typedef struct cornac_hip_recvae *cornac_hip_recvae_t;

/* recvae.py:49-84 (the model's shape) and recom_recvae.py:129, 136 (the batch rows, here never densified); all tables start
 * as zeros */
int cornac_hip_recvae_create(cornac_hip_recvae_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                             const int32_t *indices, const double *values, int hidden, int latent);
int cornac_hip_recvae_destroy(cornac_hip_recvae_t h);
/* the 53 tables from / to the host (state_dict of recvae.py:78-84) */
int cornac_hip_recvae_set_params(cornac_hip_recvae_t h, const float *const *tables);
int cornac_hip_recvae_get_params(cornac_hip_recvae_t h, float *const *tables);
/* Adam's exp_avg (m) and exp_avg_sq (v) of the 26 trainable tables and the step counters of the encoder's and the
 * decoder's optimiser (recom_recvae.py:208-209); NULL skips */
int cornac_hip_recvae_get_state(cornac_hip_recvae_t h, float *const *m, float *const *v, int64_t *t_enc, int64_t *t_dec);
/* m = v = 0, both counters 0: the two new torch.optim.Adam of recom_recvae.py:208-209 */
int cornac_hip_recvae_reset_optimizer(cornac_hip_recvae_t h);
/* recvae.py:116-117: the old encoder <- the encoder; its posterior of every user (recvae.py:35: no dropout) is computed
 * here once, with the kernels of the training forward, and read by the steps until the next call */
int cornac_hip_recvae_update_prior(cornac_hip_recvae_t h);
/* that cached posterior, mu and logvar [n_users x k] (computed first where the old tables changed); NULL skips */
int cornac_hip_recvae_get_prior_posterior(cornac_hip_recvae_t h, float *mu_out, float *logvar_out);
/* One pass of recom_recvae.py:131-145: ceil(n_users / batch_size) steps over consecutive slices of order [n_users] (every
 * user once: user_iter with shuffling), each a forward (recvae.py:94-111), the backward of the tables that step and
 * torch.optim.Adam's dense sweep (betas 0.9 / 0.999, eps 1e-8) over the encoder's tables (step_encoder), the decoder's
 * (step_decoder) or both; gradients of tables that do not step are not computed.  All steps are enqueued from this one
 * call with one synchronise at the end.  The KL weight is gamma * sum_i x_ui, or beta where gamma == 0 (recvae.py:99-103).
 * keep [nnz] is the input dropout's mask, one byte per stored entry in CSR order (read where dropout_rate > 0; kept entries
 * are scaled by 1 / (1 - dropout_rate)); eps [n_users x k] is the noise of reparameterize() itself (recvae.py:89), row =
 * user.  Either may be NULL: the device then draws it (Philox keyed by seed, the two counters' sum at the call, and entry
 * or user and column).  step_loss [steps x 3]: mll, kld and negative_elbo of each step (recvae.py:105-107); NULL skips. */
int cornac_hip_recvae_fit_epoch(cornac_hip_recvae_t h, const int32_t *order, int64_t batch_size, float lr, float gamma, float beta,
                                float dropout_rate, int step_encoder, int step_decoder, const uint8_t *keep, const float *eps,
                                uint64_t seed, double *step_loss);
/* mu_out, logvar_out [n x k]: the encoder's output for x_u without dropout (recvae.py:95 in evaluation mode, where z = mu):
 * score = decoder.bias + <mu(u), decoder.weight[i]>, so (mu, decoder.weight, decoder.bias) are a factor model's ranking
 * tables; logvar_out may be NULL */
int cornac_hip_recvae_encode_users(cornac_hip_recvae_t h, const int32_t *users, int64_t n, float *mu_out, float *logvar_out);
/* out [n x n_items] = decoder(mu(x_u)), the logits (recom_recvae.py:260-270 in evaluation mode); score_pairs: out[p] is the
 * entry items[p] of users[p]'s row (recom_recvae.py:278), the bits of the matching score_users entry */
int cornac_hip_recvae_score_users(cornac_hip_recvae_t h, const int32_t *users, int64_t n, float *out);
int cornac_hip_recvae_score_pairs(cornac_hip_recvae_t h, const int32_t *users, const int32_t *items, int64_t n, float *out);

#ifdef __cplusplus
}
#endif
#endif /* CORNAC_HIP_H_ */

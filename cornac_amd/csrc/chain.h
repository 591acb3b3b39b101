// The dataflow ("chain") driver of the deterministic kernels: mf_det_chain_kernel (mf.hip), pmf_det_chain_kernel (pmf.inc)
// and nmf_bias_chain_kernel (nmf.inc) are this protocol around their own per-rating bodies.
//
// A level schedule costs a kernel launch per link of the longest row-dependency chain (255 k links for the Netflix-shape
// MF epoch: 304 s).  Here the whole epoch is ONE persistent launch in which every rating waits for exactly what the
// sequential loop (backend_cpu.pyx:58-83) would have finished before it:
//   * every row of the OWNED side (users or items — the host picks the side whose ratings are adjacent in the stored
//     order, else the one with the longer hottest chain) belongs to one wave, and that wave applies the row's ratings
//     in their stored order: the row is read and written by one wave only — plain loads / stores;
//   * a row of the other (SHARED) side can be needed by many waves: `ver[row]` counts its finished updates, `cseq[t]` is
//     the position of rating t among that row's ratings; a rating runs when ver[row] == cseq[t], and afterwards the wave
//     drains its stores and publishes ver[row] = cseq[t] + 1.  Shared rows, their biases and the counters travel with
//     system-scope (sc0 sc1) loads and stores — they bypass the non-coherent per-XCD L2s, the valid cross-XCD form
//     without fences (MI355X_MICROARCH.md, inter-workgroup visibility);
//   * a wave never blocks on one rating: its lanes hold the cursors of 64 of its rows at a time, all 64 next ratings are
//     polled with one vector load of the counters, the ready ones are executed 64 / G per pass (one per G-lane group),
//     the chunk is polled again while anything in it moves, then the next 64 rows — cyclically over all its rows.
//     A stored order in which a row's early rating waits for another row's late one (items in random order inside
//     a user's run) therefore stalls that row only, not the wave: measured 259 s -> see DESIGN.md 1.1 for the in-order
//     form of this kernel.
// The ratings one poll finds ready are mutually independent: their owned rows are distinct (one per lane), and so are
// their shared rows — two ratings of one shared row carry different cseq, and only one can equal ver.  So a pass may run
// several of them side by side, each group doing its own ordered sum and publishing its own ver after the WAVE's stores
// have drained.
// Progress: the globally first unfinished rating is the next rating of its owned row, every earlier rating of its
// shared row is finished, and its wave visits all its rows cyclically without ever blocking — it runs.  No wave waits
// for a wave that is not resident: nothing blocks at all.  With the body stating the reference's float expression tree,
// every row sees its updates in the stored order, so the result is bit-identical to the sequential loop.
// A wave that makes no progress for `wait_bound_ticks` (a bug, never contention) raises `abort` and every wave leaves.
#pragma once
#include <algorithm>
#include <queue>
#include <vector>

#include "common.h"
#include "sgd_device.h"

namespace chip {

// the plan and the protocol state; the kernels' argument structs embed it beside their own tables and hyper-parameters
struct ChainArgs {
    const int64_t *wrow_ptr;        // [W + 1] rows of wave w = [wrow_ptr[w], wrow_ptr[w + 1])
    const int32_t *row_id;          // owned-side id of a row
    const int64_t *row_end;         // end of the row's ratings in csid / cseq / cr
    int64_t *row_cur;               // next rating of the row (reset to the row's begin every epoch)
    const int32_t *csid, *cseq;     // shared-side id of a rating, its position among that row's ratings
    const float *cr;
    unsigned int *ver;              // [rows of the shared side] finished updates of the row in this epoch
    unsigned int *abort;            // [8]: [0] a wave gave up, [1] which
    long long wait_bound_ticks;     // of the 100 MHz real-time counter
};

// one rating of one pass, as its lane group sees it
struct ChainPass {
    bool act;           // this lane group has a rating in this pass
    int lg;             // the lane's index in its group
    int32_t oid, sid;   // owned-side id, shared-side id
    float r;
    int64_t pos;        // of the rating in csid / cseq / cr
};

__device__ __forceinline__ float load_f32_sys(const float *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void store_f32_sys(float *p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ double load_f64_sys(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void store_f64_sys(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// lane l's value to every lane that names l: with one group per wave l is uniform (v_readlane)
template <int G>
__device__ __forceinline__ int chain_bcast(int v, int l) {
    return G == kWave ? __builtin_amdgcn_readlane(v, l) : __shfl(v, l, kWave);
}

// The whole protocol around `body(ChainPass)`, which does one rating's loads, expression tree and stores with the
// lanes of its group (shared-side rows through the *_sys accesses).  G lanes per rating: 64 / G ready ratings per pass.
template <int G, class Body>
__device__ __forceinline__ void chain_run(const ChainArgs &c, Body &&body) {
    constexpr int TPW = kWave / G;
    const int lane = lane_id();
    const int grp = lane / G, lg = lane & (G - 1);
    const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t q0 = c.wrow_ptr[w], q1 = c.wrow_ptr[w + 1];
    unsigned long long t_idle = 0;  // real-time stamp of the first fruitless sweep in a row (0: progressing)
    unsigned int idle_sweeps = 0;
    bool give_up = false;
    while (!give_up) {
        bool unfinished = false, progressed = false;
        for (int64_t base = q0; base < q1; base += kWave) {
            const int64_t q = base + lane;
            const bool mine = q < q1;
            int64_t cur = mine ? c.row_cur[q] : 0;
            const int64_t rend = mine ? c.row_end[q] : 0;
            const int32_t oid = mine ? c.row_id[q] : 0;
            for (;;) {
                // ---- poll the next rating of up to 64 rows at once ----
                const bool has = mine && cur < rend;
                const int32_t sid = has ? c.csid[cur] : 0;
                const unsigned int seq = has ? (unsigned int)c.cseq[cur] : 0u;
                const unsigned int v = has ? __hip_atomic_load(c.ver + sid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ~0u;
                unsigned long long ready = __ballot(has && v == seq);
                if (!ready) break;
                asm volatile("" ::: "memory");  // (compiler: the row loads below stay behind the poll; the hardware issues in order)
                progressed = true;
                const float rr = has ? c.cr[cur] : 0.f;
                while (ready) {
                    // ---- this pass: the next ready ratings, one per lane group ----
                    int l = lane;
                    bool act = false;
                    unsigned long long taken = 0ull;
#pragma unroll
                    for (int g = 0; g < TPW; ++g) {
                        if (ready) {
                            const int lj = __builtin_ctzll(ready);
                            ready &= ready - 1;
                            taken |= 1ull << lj;
                            if (TPW == 1 || grp == g) {
                                l = lj;
                                act = true;
                            }
                        }
                    }
                    ChainPass p;
                    p.act = act;
                    p.lg = lg;
                    p.oid = chain_bcast<G>(oid, l);
                    p.sid = chain_bcast<G>(sid, l);
                    p.r = __builtin_bit_cast(float, chain_bcast<G>(__builtin_bit_cast(int, rr), l));
                    p.pos = (int64_t)(((unsigned long long)(unsigned int)chain_bcast<G>((int)(cur >> 32), l) << 32) |
                                      (unsigned int)chain_bcast<G>((int)cur, l));
                    const unsigned int sq = (unsigned int)chain_bcast<G>((int)seq, l);
                    body(p);
                    // ---- publish: every store of this wave has left before any of its counters moves ----
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (act && lg == 0) __hip_atomic_store(c.ver + p.sid, sq + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if ((taken >> lane) & 1ull) ++cur;
                }
            }
            if (mine) c.row_cur[q] = cur;
            unfinished = unfinished || __ballot(mine && cur < rend) != 0ull;
        }
        if (!unfinished) break;
        if (progressed) {
            t_idle = 0;
            idle_sweeps = 0;
            continue;
        }
        // nothing of this wave can run yet: back off (longer the longer it lasts) and watch the bound
        ++idle_sweeps;
        if (idle_sweeps < 8) __builtin_amdgcn_s_sleep(8);
        else if (idle_sweeps < 64) __builtin_amdgcn_s_sleep(64);
        else __builtin_amdgcn_s_sleep(127);
        if ((idle_sweeps & 255u) == 0) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (t_idle == 0) t_idle = now;
            int bad = 0;
            if (lane == 0 && (now - t_idle > (unsigned long long)c.wait_bound_ticks ||
                              __hip_atomic_load(c.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))) {
                if (atomicCAS(c.abort, 0u, 1u) == 0u) c.abort[1] = (unsigned int)w;
                bad = 1;
            }
            give_up = __builtin_amdgcn_readfirstlane(bad) != 0;
        }
    }
}

// ---- host: the plan and the launch ---------------------------------------------------------------------------------------
struct ChainPlan {
    DevBuf<int64_t> wrow_ptr, row_beg, row_end, row_cur;
    DevBuf<int32_t> row_id;
    DevBuf<unsigned int> ver, abort;
    int grid = 0;        // workgroups of the cooperative launch (0: no plan)
    size_t n_rows = 0;   // non-empty owned rows
};

// Owned rows -> W waves, heaviest first onto the least loaded wave; empty rows take no part; a wave's rows in the order
// of their first rating.  cnt[r]: ratings of row r, first[r]: stored position of its first one.  Fills wrow_ptr [W + 1]
// and row_id (the rows in plan order).
static void chain_deal(const std::vector<int64_t> &cnt, const std::vector<int64_t> &first, int64_t W,
                       std::vector<int64_t> &wrow_ptr, std::vector<int32_t> &row_id) {
    std::vector<int32_t> order(cnt.size());
    for (size_t r = 0; r < order.size(); ++r) order[r] = (int32_t)r;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cnt[(size_t)x] > cnt[(size_t)y]; });
    typedef std::pair<int64_t, int64_t> LW;
    std::priority_queue<LW, std::vector<LW>, std::greater<LW>> heap;
    for (int64_t w = 0; w < W; ++w) heap.push(LW(0, w));
    std::vector<std::vector<int32_t>> wrows((size_t)W);
    for (int32_t r : order) {
        if (cnt[(size_t)r] == 0) continue;
        LW top = heap.top();
        heap.pop();
        wrows[(size_t)top.second].push_back(r);
        top.first += cnt[(size_t)r];
        heap.push(top);
    }
    wrow_ptr.assign((size_t)W + 1, 0);
    row_id.clear();
    for (int64_t w = 0; w < W; ++w) {
        std::sort(wrows[(size_t)w].begin(), wrows[(size_t)w].end(), [&](int32_t x, int32_t y) { return first[(size_t)x] < first[(size_t)y]; });
        row_id.insert(row_id.end(), wrows[(size_t)w].begin(), wrows[(size_t)w].end());
        wrow_ptr[(size_t)w + 1] = (int64_t)row_id.size();
    }
}

// the dealt rows with their rating ranges onto the device, and the protocol state: cursors, n_shared counters, abort
static void chain_upload(ChainPlan &pl, int grid, const std::vector<int64_t> &wrow_ptr, const std::vector<int32_t> &row_id,
                         const std::vector<int64_t> &row_beg, const std::vector<int64_t> &row_end, int64_t n_shared,
                         hipStream_t stream) {
    const size_t n_rows = row_id.size(), cap = std::max<size_t>(n_rows, 1);
    pl.wrow_ptr.alloc(wrow_ptr.size());
    pl.row_id.alloc(cap); pl.row_beg.alloc(cap); pl.row_end.alloc(cap); pl.row_cur.alloc(cap);
    pl.ver.alloc((size_t)n_shared);
    pl.abort.alloc(8);
    pl.wrow_ptr.upload(wrow_ptr.data(), wrow_ptr.size(), stream);
    if (n_rows) {
        pl.row_id.upload(row_id.data(), n_rows, stream);
        pl.row_beg.upload(row_beg.data(), n_rows, stream);
        pl.row_end.upload(row_end.data(), n_rows, stream);
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    pl.n_rows = n_rows;
    pl.grid = grid;
}

static ChainArgs chain_args(const ChainPlan &pl, const int32_t *csid, const int32_t *cseq, const float *cr) {
    ChainArgs c;
    c.wrow_ptr = pl.wrow_ptr.p; c.row_id = pl.row_id.p; c.row_end = pl.row_end.p; c.row_cur = pl.row_cur.p;
    c.csid = csid; c.cseq = cseq; c.cr = cr;
    c.ver = pl.ver.p; c.abort = pl.abort.p;
    c.wait_bound_ticks = (long long)prof_env_int("CORNAC_HIP_MF_CHAIN_WAIT_S", 120) * 100000000ll;
    return c;
}

// One epoch of a dataflow kernel over `pl`.  The waves wait for each other (per-row hand-over counters): every workgroup
// of the grid has to be resident.  A cooperative launch makes that the runtime's business — it refuses a grid that cannot
// be co-resident instead of letting the resident half spin on the other half until the time bound.  Returns false on
// that refusal: nothing has run, the caller takes the level schedule.  Any other status is a real launch error.
template <class Args>
static bool chain_launch(hipStream_t stream, ChainPlan &pl, void (*kernel)(const Args), Args *args, const char *name) {
    HIP_CHECK(hipMemsetAsync(pl.ver.p, 0, pl.ver.n * sizeof(unsigned int), stream));
    HIP_CHECK(hipMemsetAsync(pl.abort.p, 0, 8 * sizeof(unsigned int), stream));
    if (pl.n_rows)
        HIP_CHECK(hipMemcpyAsync(pl.row_cur.p, pl.row_beg.p, pl.n_rows * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
    void *kargs[] = {(void *)args};
    const hipError_t st = hipLaunchCooperativeKernel((const void *)kernel, dim3(pl.grid), dim3(kBlock), kargs, 0, stream);
    if (st == hipErrorCooperativeLaunchTooLarge) {
        (void)hipGetLastError();
        return false;
    }
    HIP_CHECK(st);
    unsigned int ab[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(ab, pl.abort.p, sizeof ab, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (ab[0]) fail(CORNAC_HIP_ERR_HIP, "%s: wave %u made no progress for its time bound (internal error)", name, ab[1]);
    return true;
}

}  // namespace chip

"""TEST INFRASTRUCTURE ONLY — Python face of the CPU oracle (oracle/cornac_oracle.c).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this.
It restates, on the CPU, what the reference's seeded (num_threads == 1) path
computes, end to end:

  * BPROracle / WBPROracle  -> cornac/models/bpr/recom_bpr.pyx:145-206, recom_wbpr.pyx:103-144
  * MFOracle               -> cornac/models/mf/recom_mf.py:138-209 + backend_cpu.pyx:35-97
  * fast_dot / score / rank -> cornac/utils/fast_dot.pyx:40-43, recom_bpr.pyx:272-297,
                               recom_mf.py:254-286, cornac/models/recommender.py:476-530

The initialisers use NumPy's RandomState exactly like the reference
(cornac/utils/init_utils.py:33-57 `uniform`, :60-82 `normal`) so seeded runs
start from bit-identical factors.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libcornac_oracle.so")
_lib = None

f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


def build(force=False):
    src = os.path.join(_HERE, "cornac_oracle.c")
    fast = _SO.replace("libcornac_oracle.so", "libcornac_oracle_fast.so")
    if force or not os.path.exists(_SO) or not os.path.exists(fast) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []))
    return _SO


_fast = None


def fast_lib():
    """same source compiled with the reference's flags (-O3 -ffast-math): CPU-baseline timing only"""
    global _fast
    if _fast is None:
        build()
        _fast = _bind(C.CDLL(_SO.replace("libcornac_oracle.so", "libcornac_oracle_fast.so")))
    return _fast


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = _bind(C.CDLL(_SO))
    return _lib


def _bind(L):
    if True:
        L.oracle_mt_seed.argtypes = [C.c_void_p, C.c_uint32]
        L.oracle_mt_next.argtypes = [C.c_void_p]
        L.oracle_mt_next.restype = C.c_uint32
        L.oracle_boost_uniform.argtypes = [C.c_void_p, C.c_uint64]
        L.oracle_boost_uniform.restype = C.c_int64
        L.oracle_boost_uniform_fill.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, i64p]
        L.oracle_mt_fill_raw.argtypes = [C.c_void_p, C.c_int64, u32p]
        L.oracle_bpr_epoch_seq.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, i32p, i32p,
                                           i32p, i32p, f32p, f32p, f32p, C.c_int, C.c_float, C.c_float, C.c_int,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
        L.oracle_bpr_epoch_seq_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, i32p, i32p,
                                               i32p, i32p, f64p, f64p, f64p, C.c_int, C.c_double, C.c_double, C.c_int,
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oracle_bpr_epoch_omp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_int64, i32p,
                                           i32p, i32p, i32p, f32p, f32p, f32p, C.c_int, C.c_float, C.c_float,
                                           C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oracle_vebpr_epoch_seq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, i32p, i32p, i32p,
                                             i32p, i32p, f32p, f32p, C.c_int, C.c_float, C.c_float, C.c_float,
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oracle_vebpr_epoch_seq_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, i32p, i32p, i32p,
                                                 i32p, i32p, f64p, f64p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oracle_mf_fit.argtypes = [i64p, i64p, f32p, C.c_int64, f32p, f32p, f32p, f32p, C.c_int, C.c_float,
                                    C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.oracle_fast_dot.argtypes = [f32p, f32p, f32p, C.c_int64, C.c_int, C.c_int]
        L.oracle_score_block.argtypes = [f32p, f32p, C.c_void_p, C.c_void_p, i32p, C.c_int64, C.c_int64, C.c_int,
                                         f32p]
        L.oracle_philox4x32.argtypes = [C.c_uint32] * 6 + [u32p]
        L.oracle_hogwild_sample.argtypes = [C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32,
                                            i64p, i64p]
        L.oracle_hogwild_sample_owned.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_int64, C.c_int64, i64p, i64p]
        L.oracle_strata_rot.argtypes = [C.c_uint32, C.c_uint32]
        L.oracle_strata_rot.restype = C.c_uint32
        L.oracle_strata_key.argtypes = [C.c_uint64, C.c_uint32]
        L.oracle_strata_key.restype = C.c_uint32
        L.oracle_strata_partitions.argtypes = [C.c_uint32, C.c_int64, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]
        L.oracle_strata_sample.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, i64p, i64p]
        L.oracle_strata_sample.restype = C.c_int64
        L.oracle_ldsbin_key.argtypes = [C.c_uint64, C.c_uint32]
        L.oracle_ldsbin_key.restype = C.c_uint32
        L.oracle_ldsbin_hot_shuffle_key.argtypes = [C.c_uint32]
        L.oracle_ldsbin_hot_shuffle_key.restype = C.c_uint32
        L.oracle_ldsbin_deal.argtypes = [C.c_uint32] * 6 + [i32p, i32p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_ldsbin_deal.restype = None
        L.oracle_ldsbin_layout.argtypes = [C.c_uint32] * 4 + [i32p, C.c_void_p, C.c_void_p]
        L.oracle_ldsbin_layout.restype = None
        L.oracle_ldsbin_epoch_skips.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, i32p,
                                                i32p, i32p, i32p, i32p, C.c_uint32, i32p, i32p, C.POINTER(C.c_int64),
                                                C.c_void_p, C.c_void_p, C.c_int]
        L.oracle_ldsbin_epoch_skips.restype = C.c_int64
        L.oracle_ldsbin_epoch_skips_range.argtypes = list(L.oracle_ldsbin_epoch_skips.argtypes) + [C.c_uint32, C.c_uint32]
        L.oracle_ldsbin_epoch_skips_range.restype = C.c_int64
        L.oracle_ldsbin_draws.argtypes = list(L.oracle_ldsbin_epoch_skips_range.argtypes) + [C.c_uint64] * 3 + [C.c_void_p] * 5 + [
            C.c_int64, C.POINTER(C.c_int64)]
        L.oracle_ldsbin_draws.restype = C.c_int64
        f64p_ = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
        L.oracle_bpr_apply_seq_f64.argtypes = [i64p, i64p, i64p, i64p, C.c_int64, f64p_, f64p_, f64p_, C.c_int, C.c_double,
                                               C.c_double, C.c_int]
        L.oracle_bpr_apply_seq_f64.restype = None
        L.oracle_bpr_jacobi_f64.argtypes = [i64p, i64p, i64p, C.c_int64, f32p, f32p, f32p, C.c_int, C.c_double, C.c_double,
                                            C.c_int] + [f64p_] * 6 + [i64p] * 3 + [f64p_] * 2
        L.oracle_bpr_jacobi_f64.restype = None
        L.oracle_mf_apply_seq_f64.argtypes = [i64p, i64p, f32p, i64p, C.c_int64, f64p_, f64p_, f64p_, f64p_, C.c_int, C.c_double,
                                              C.c_double, C.c_double, C.c_int]
        L.oracle_mf_apply_seq_f64.restype = None
        L.oracle_mf_jacobi_f64.argtypes = [i64p, i64p, f32p, C.c_int64, f32p, f32p, f32p, f32p, C.c_int, C.c_double, C.c_double,
                                           C.c_double, C.c_int, C.c_double] + [f64p_] * 8 + [i64p] * 4 + [f64p_]
        L.oracle_mf_jacobi_f64.restype = None
        L.oracle_vebpr_hogwild_sample.argtypes = [C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32,
                                                  i64p, u32p, i64p]
        L.oracle_vebpr_hogwild_sample.restype = None
        L.oracle_vebpr_hogwild_sample_owned.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                        C.c_int64, C.c_int64, i64p, u32p, i64p]
        L.oracle_vebpr_hogwild_sample_owned.restype = None
        L.oracle_vebpr_apply_seq_f64.argtypes = [i64p] * 5 + [C.c_int64, f64p_, f64p_, C.c_int, C.c_double, C.c_double,
                                                              C.c_double, C.c_int, C.c_int, C.c_int64, C.c_double]
        L.oracle_vebpr_apply_seq_f64.restype = None
        L.oracle_vebpr_jacobi_f64.argtypes = [i64p] * 4 + [C.c_int64, f32p, f32p, C.c_int, C.c_double, C.c_double,
                                                           C.c_double] + [f64p_] * 4 + [i64p] * 2 + [f64p_]
        L.oracle_vebpr_jacobi_f64.restype = None
        L.oracle_num_threads.restype = C.c_int
        L.oracle_sizeof_mt.restype = C.c_int
    return L


class MT19937:
    """boost::random::mt19937 (recom_bpr.pxd:26-32)."""

    def __init__(self, seed):
        self.buf = C.create_string_buffer(lib().oracle_sizeof_mt())
        lib().oracle_mt_seed(self.buf, int(seed) & 0xFFFFFFFF)

    @property
    def ptr(self):
        return C.cast(self.buf, C.c_void_p)

    def raw(self, n):
        out = np.empty(n, np.uint32)
        lib().oracle_mt_fill_raw(self.ptr, n, out)
        return out

    def uniform_int(self, hi, n):
        out = np.empty(n, np.int64)
        if lib().oracle_boost_uniform_fill(self.ptr, int(hi), n, out) != 0:
            raise ValueError("range >= 2**32 is not reachable in the reference")
        return out


def rngvector_seed(seed):
    """RNGVector(1, rows, seed): thread 0's mt19937 seed = RandomState(seed).randint(2**31)
    (recom_bpr.pyx:55-59)."""
    return int(np.random.RandomState(seed).randint(2 ** 31))


def rngvector_seeds(seed, num_threads):
    rng = np.random.RandomState(seed)
    return [int(rng.randint(2 ** 31)) for _ in range(num_threads)]


def _uniform(shape, rng, dtype=np.float32):
    # cornac/utils/init_utils.py:33-57  uniform(shape, low=0, high=1).astype(dtype)
    return rng.uniform(0.0, 1.0, shape).astype(dtype)


def _normal(shape, rng, std, dtype=np.float32):
    # cornac/utils/init_utils.py:60-82
    return rng.normal(0.0, std, shape).astype(dtype)


def csr_arrays(train_set):
    X = train_set.matrix
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    user_ids = np.repeat(np.arange(train_set.num_users), np.ediff1d(indptr)).astype(np.int32)
    return indptr, indices, user_ids


class BPROracle:
    """Seeded BPR exactly as the reference runs it with `seed is not None`."""

    weighted = False  # WBPR: one shared stream, negatives drawn from X.indices

    def __init__(self, k=10, max_iter=100, learning_rate=0.001, lambda_reg=0.01, use_bias=True, seed=None,
                 init_params=None):
        self.k, self.max_iter, self.lr, self.reg, self.use_bias = int(k), max_iter, learning_rate, lambda_reg, use_bias
        self.seed = seed
        self.rng = np.random.RandomState(seed)  # created in __init__ (recom_bpr.pyx:130)
        ip = init_params or {}
        self.u_factors, self.i_factors, self.i_biases = ip.get("U"), ip.get("V"), ip.get("Bi")
        self.record = None

    def _init(self, train_set):
        # Recommender.total_users/total_items = len(uid_map)/len(iid_map) (recommender.py:150-158)
        nu, ni = len(train_set.uid_map), len(train_set.iid_map)
        if self.u_factors is None:
            self.u_factors = (_uniform((nu, self.k), self.rng) - 0.5) / self.k
        if self.i_factors is None:
            self.i_factors = (_uniform((ni, self.k), self.rng) - 0.5) / self.k
        if self.i_biases is None or not self.use_bias:
            self.i_biases = np.zeros(ni, np.float32)
        # `_fit_sgd` is a fused-type function (recom_bpr.pyx:211-214): three float64 tables train in double, three
        # float32 tables in float; a mix fails the buffer check (the reference raises ValueError)
        kinds = {np.asarray(getattr(self, n)).dtype for n in ("u_factors", "i_factors", "i_biases")}
        if kinds == {np.dtype(np.float64)}:
            self.dtype = np.float64
        elif kinds == {np.dtype(np.float32)}:
            self.dtype = np.float32
        else:
            raise ValueError("Buffer dtype mismatch: U, V and Bi must share one dtype")
        for n in ("u_factors", "i_factors", "i_biases"):
            setattr(self, n, np.ascontiguousarray(getattr(self, n), dtype=self.dtype))

    def fit(self, train_set, record=False):
        L = lib()
        self._init(train_set)
        indptr, indices, user_ids = csr_arrays(train_set)
        nnz = len(user_ids)
        if self.weighted:
            g = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
            gp = gn = g
            neg_ids, neg_hi = indices, nnz - 1
        else:
            neg_ids = np.arange(train_set.num_items, dtype=np.int32)
            gp = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
            gn = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
            neg_hi = train_set.num_items - 1
        self.correct, self.skipped = [], []
        if record:
            self.record = []
        for _ in range(self.max_iter):
            c, s = C.c_int64(), C.c_int64()
            rec = [None, None, None]
            if record:
                rec = [np.empty(nnz, np.int64), np.empty(nnz, np.int64), np.empty(nnz, np.uint8)]
            if self.dtype == np.float64:
                assert not record, "the float64 restatement keeps no draw record"
                rc = L.oracle_bpr_epoch_seq_f64(gp.ptr, gn.ptr, nnz - 1, neg_hi, nnz, user_ids, indices, neg_ids, indptr,
                                                self.u_factors, self.i_factors, self.i_biases, self.k, self.lr, self.reg,
                                                int(self.use_bias), C.byref(c), C.byref(s))
            else:
                rc = L.oracle_bpr_epoch_seq(gp.ptr, gn.ptr, nnz - 1, neg_hi, nnz, user_ids, indices, neg_ids, indptr,
                                            self.u_factors, self.i_factors, self.i_biases, self.k, self.lr, self.reg,
                                            int(self.use_bias), C.byref(c), C.byref(s),
                                            *[r.ctypes.data if r is not None else None for r in rec])
            if rc != 0:
                raise ValueError("oracle_bpr_epoch_seq failed")
            self.correct.append(c.value)
            self.skipped.append(s.value)
            if record:
                self.record.append(rec)
        return self

    def score(self, user_idx, mode=1):
        out = np.copy(self.i_biases)
        if out.dtype == np.float64:  # fast_dot's ddot variant (fast_dot.pyx:25-43); the BLAS summation order is not pinned
            return out + self.i_factors @ self.u_factors[user_idx]
        lib().oracle_fast_dot(self.u_factors[user_idx], self.i_factors, out, len(out), self.k, mode)
        return out


class WBPROracle(BPROracle):
    weighted = True


class VEBPROracle:
    """Seeded VEBPR (cornac/models/bpr/recom_vebpr.pyx:100-209): train_set must expose `matrix`
    (purchases) and `view_matrix` (views minus purchases, sorted CSR)."""

    def __init__(self, k=10, max_iter=100, learning_rate=0.01, lambda_reg=0.1, alpha=0.5, seed=None,
                 init_params=None):
        self.k, self.max_iter, self.lr, self.reg, self.alpha = int(k), max_iter, learning_rate, lambda_reg, float(alpha)
        self.rng = np.random.RandomState(seed)
        ip = init_params or {}
        self.u_factor, self.i_factor = ip.get("U"), ip.get("V")

    def fit(self, train_set):
        L = lib()
        nu, ni = len(train_set.uid_map), len(train_set.iid_map)
        if self.u_factor is None:
            self.u_factor = (_uniform((nu, self.k), self.rng) - 0.5) / self.k
        if self.i_factor is None:
            self.i_factor = (_uniform((ni, self.k), self.rng) - 0.5) / self.k
        # float64 tables (both given through init_params) train in double: recom_vebpr.pyx:219 is a fused-type function
        f64 = np.asarray(self.u_factor).dtype == np.float64 and np.asarray(self.i_factor).dtype == np.float64
        dt = np.float64 if f64 else np.float32
        self.u_factor = np.ascontiguousarray(self.u_factor, dt)
        self.i_factor = np.ascontiguousarray(self.i_factor, dt)
        indptr, indices, user_ids = csr_arrays(train_set)
        Vw = train_set.view_matrix
        v_indptr = np.ascontiguousarray(Vw.indptr, np.int32)
        v_indices = np.ascontiguousarray(Vw.indices, np.int32)
        if len(v_indices) == 0:
            v_indices = np.zeros(1, np.int32)
        gp = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
        gv = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
        gn = MT19937(rngvector_seed(self.rng.randint(2 ** 31)))
        self.correct, self.skipped = [], []
        for _ in range(self.max_iter):
            c, s = C.c_int64(), C.c_int64()
            (L.oracle_vebpr_epoch_seq_f64 if f64 else L.oracle_vebpr_epoch_seq)(
                gp.ptr, gv.ptr, gn.ptr, len(user_ids), train_set.num_items, user_ids, indices, indptr, v_indices, v_indptr,
                self.u_factor, self.i_factor, self.k, self.lr, self.reg, self.alpha, C.byref(c), C.byref(s))
            self.correct.append(c.value)
            self.skipped.append(s.value)
        return self


def bpr_hogwild_epochs(indptr, indices, user_ids, n_items, U, V, B, k, lr, reg, use_bias, seed, num_threads,
                       epochs, num_samples=None, fast=True):
    """The reference's unseeded multi-thread path (racy), for the CPU throughput baseline.
    num_samples: draws per epoch (default nnz, like the reference)."""
    L = fast_lib() if fast else lib()
    nnz = len(user_ids)
    n_draw = nnz if num_samples is None else int(num_samples)
    T = num_threads
    sz = L.oracle_sizeof_mt()
    rng = np.random.RandomState(seed)
    bufs, keep = [], []
    for _ in range(2):
        raw = C.create_string_buffer(sz * T + 64)
        base = (C.addressof(raw) + 63) & ~63  # cache-line aligned array of T engines
        for t, s in enumerate(rngvector_seeds(rng.randint(2 ** 31), T)):
            L.oracle_mt_seed(C.c_void_p(base + t * sz), s)
        keep.append(raw)
        bufs.append(C.c_void_p(base))
    neg_ids = np.arange(n_items, dtype=np.int32)
    tot_c = tot_s = 0
    for _ in range(epochs):
        c, s = C.c_int64(), C.c_int64()
        L.oracle_bpr_epoch_omp(bufs[0], bufs[1], T, nnz - 1, n_items - 1, n_draw, user_ids, indices, neg_ids, indptr,
                               U, V, B, k, lr, reg, int(use_bias), C.byref(c), C.byref(s))
        tot_c += c.value
        tot_s += s.value
    return tot_c, tot_s


class MFOracle:
    """MF(backend='cpu') seeded (recom_mf.py:138-209)."""

    def __init__(self, k=10, max_iter=20, learning_rate=0.01, lambda_reg=0.02, use_bias=True, early_stop=False,
                 seed=None, init_params=None, num_threads=1):
        self.k, self.max_iter, self.lr, self.reg = int(k), max_iter, learning_rate, lambda_reg
        self.use_bias, self.early_stop, self.seed, self.num_threads = use_bias, early_stop, seed, num_threads
        ip = init_params or {}
        self.u_factors, self.i_factors = ip.get("U"), ip.get("V")
        self.u_biases, self.i_biases = ip.get("Bu"), ip.get("Bi")

    def fit(self, train_set):
        rng = np.random.RandomState(self.seed)
        nu, ni = train_set.num_users, train_set.num_items
        if self.u_factors is None:
            self.u_factors = _normal((nu, self.k), rng, 0.01)
        if self.i_factors is None:
            self.i_factors = _normal((ni, self.k), rng, 0.01)
        if self.u_biases is None:
            self.u_biases = np.zeros(nu, np.float32)
        if self.i_biases is None:
            self.i_biases = np.zeros(ni, np.float32)
        for n in ("u_factors", "i_factors", "u_biases", "i_biases"):
            setattr(self, n, np.ascontiguousarray(getattr(self, n), dtype=np.float32))
        self.global_mean = np.float32(train_set.global_mean if self.use_bias else 0.0)
        rid, cid, val = train_set.uir_tuple
        rid = np.ascontiguousarray(rid, np.int64)
        cid = np.ascontiguousarray(cid, np.int64)
        val = np.ascontiguousarray(val, np.float32)
        self.loss = np.zeros(max(self.max_iter, 1), np.float32)
        self.epochs_run = lib().oracle_mf_fit(rid, cid, val, len(val), self.u_factors, self.i_factors, self.u_biases,
                                              self.i_biases, self.k, self.lr, self.reg, float(self.global_mean),
                                              self.max_iter, self.num_threads, int(self.use_bias),
                                              int(self.early_stop), self.loss.ctypes.data)
        return self

    def score(self, user_idx, mode=1):
        out = (self.global_mean + self.i_biases).astype(np.float32)
        out += self.u_biases[user_idx]
        lib().oracle_fast_dot(self.u_factors[user_idx], self.i_factors, out, len(out), self.k, mode)
        return out


def fast_dot(vec, mat, output, mode=0):
    """output += mat @ vec in place (cornac/utils/fast_dot.pyx:40-43)."""
    vec = np.ascontiguousarray(vec, np.float32)
    mat = np.ascontiguousarray(mat, np.float32)
    assert output.dtype == np.float32 and output.flags.c_contiguous
    lib().oracle_fast_dot(vec, mat, output, mat.shape[0], mat.shape[1], mode)


def score_block(U, V, item_base, user_base, users):
    users = np.ascontiguousarray(users, np.int32)
    out = np.empty((len(users), V.shape[0]), np.float32)
    ib = None if item_base is None else np.ascontiguousarray(item_base, np.float32).ctypes.data
    ub = None if user_base is None else np.ascontiguousarray(user_base, np.float32).ctypes.data
    lib().oracle_score_block(np.ascontiguousarray(U, np.float32), np.ascontiguousarray(V, np.float32), ib, ub, users,
                             len(users), V.shape[0], V.shape[1], out)
    return out


def rank(all_item_scores, num_items, total_items, item_indices=None, k=-1):
    """Recommender.rank after score() (cornac/models/recommender.py:503-530).

    The reference's tie order is unspecified (np.argsort default / argpartition;
    acknowledged in tests/cornac/models/test_recommender.py:89-93).  The oracle pins
    it: descending score, ties by descending position in `item_indices` (= a
    stable ascending argsort read backwards).  With k != -1 only the first k
    entries are defined (the reference leaves the tail in argpartition order).
    """
    known = np.asarray(all_item_scores)
    if len(known) != total_items:
        full = np.ones(total_items) * np.min(known)
        full[:num_items] = known
        known = full
    item_indices = np.arange(num_items) if item_indices is None else np.asarray(item_indices)
    item_scores = known[item_indices]
    order = np.argsort(item_scores, kind="stable")[::-1]
    ranked = item_indices[order]
    if k != -1:
        ranked = ranked[:k]
    return ranked, item_scores


def hogwild_sample(seed, epoch, s0, n, n_pos, n_neg):
    ii = np.empty(n, np.int64)
    jj = np.empty(n, np.int64)
    lib().oracle_hogwild_sample(int(seed), int(epoch), int(s0), int(n), int(n_pos), int(n_neg), ii, jj)
    return ii, jj


def strata_key(seed, epoch):
    return int(lib().oracle_strata_key(int(seed), int(epoch)))


def strata_partitions(key, n_items):
    """partition (0..7) of every popularity rank under the epoch key (csrc/bpr_strata.inc)"""
    out = np.empty(n_items, np.uint8)
    lib().oracle_strata_partitions(int(key), int(n_items), out)
    return out


def strata_sample(seed, epoch, key, wave_id, p, length, n_items):
    """(index into the wave's bucket p, popularity rank of the negative) for the bucket's `length` draws"""
    r = np.empty(length, np.int64)
    code = np.empty(length, np.int64)
    n = lib().oracle_strata_sample(int(seed), int(epoch), int(key), int(wave_id), int(p), int(length), int(n_items), r, code)
    return r[:n], code[:n]


def strata_buckets(wave_ptr, own_u, own_i, deg, key, n_hot):
    """CPU restatement of strata_bucket_kernel: every wave slice stably re-ordered by the partition of its items.
    Returns (sptr [8 W + 1], rec_u, rec_i with bit 31 = hot, rank_item)."""
    n_items = len(deg)
    rank_item = np.argsort(-deg.astype(np.int64), kind="stable").astype(np.int32)
    item_rank = np.empty(n_items, np.int64)
    item_rank[rank_item] = np.arange(n_items)
    part_rank = strata_partitions(key, n_items)
    W = len(wave_ptr) - 1
    code = item_rank[own_i]
    part = part_rank[code].astype(np.int64)
    wave_of = np.repeat(np.arange(W, dtype=np.int64), np.diff(wave_ptr))
    order = np.argsort(wave_of * 8 + part, kind="stable")
    counts = np.bincount(wave_of * 8 + part, minlength=8 * W)
    sptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rec_u = own_u[order]
    rec_i = own_i[order].astype(np.int64)
    rec_i = np.where(code[order] < n_hot, rec_i | 0x80000000, rec_i).astype(np.uint32).view(np.int32)
    return sptr, rec_u, rec_i, rank_item


def strata_n_hot(deg, nnz, n_items, hot_permille=120, hot_min_mult_x100=200):
    """the hot-set rule of csrc/bpr.hip build_item_ranks in the same double arithmetic: the leading popularity ranks whose
    expected touches per epoch (degree + the uniform share nnz / n_items of the negative draws) are at least
    hot_min_mult_x100 / 100 times the mean row's and that together stay within hot_permille / 1000 of all 2 nnz item-row
    touches; the walk stops at the first rank that fails either condition"""
    deg = np.asarray(deg, np.int64)
    order = np.argsort(-deg, kind="stable")
    neg_share = float(nnz) / float(n_items)
    mean_touch = 2.0 * neg_share
    cap = 2.0 * float(nnz) * int(hot_permille) / 1000.0
    cum, n_hot = 0.0, 0
    for r in range(int(n_items)):
        touch = float(deg[order[r]]) + neg_share
        if touch * 100.0 < mean_touch * int(hot_min_mult_x100) or cum + touch > cap:
            break
        cum += touch
        n_hot = r + 1
    return n_hot


def strata_unr(k):
    """triplets per wave step of the strata kernel the dispatcher returns for k (csrc/bpr.hip pick_strata_kernel)"""
    return 4 if k <= 64 else 2 if k <= 192 else 1


def _strata_triplets(seed, epoch, s_begin, n, indptr, indices, n_items, ownership, k, hot_permille, hot_min_mult_x100,
                     rehash_period):
    nnz = len(indices)
    first_phase = lambda s: (8 * int(s) + nnz - 1) // nnz
    p_lo, p_hi = first_phase(s_begin), 8 if s_begin + n >= nnz else first_phase(s_begin + n)
    wave_ptr, own_u, own_i = ownership
    W = len(wave_ptr) - 1
    deg = np.bincount(indices, minlength=n_items)
    n_hot = strata_n_hot(deg, nnz, n_items, hot_permille, hot_min_mult_x100)
    key = strata_key(seed, int(epoch) // max(1, int(rehash_period)))
    sptr, rec_u, rec_i, rank_item = strata_buckets(wave_ptr, own_u, own_i, deg, key, n_hot)
    unr = strata_unr(k)
    cols = {name: [] for name in ("su", "si", "code", "wave", "phase", "t")}
    for ph in range(p_lo, p_hi):
        for w in range(W):
            p = ((w // 4) % 8 + ph) % 8
            base, length = int(sptr[8 * w + p]), int(sptr[8 * w + p + 1] - sptr[8 * w + p])
            if length == 0:
                continue
            r, code = strata_sample(seed, epoch, key, w, p, length, n_items)
            m = len(r)  # (0 where the partition has no item: the device counts the bucket's draws as skipped)
            assert m == length, "a partition without items: not a case for this restatement"
            cols["su"].append(rec_u[base + r])
            cols["si"].append(rec_i[base + r])
            cols["code"].append(code)
            cols["wave"].append(np.full(m, w, np.int64))
            cols["phase"].append(np.full(m, ph, np.int64))
            cols["t"].append(np.arange(m, dtype=np.int64))
    cat = {name: (np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64)) for name, v in cols.items()}
    su, si, code = cat["su"], cat["si"], cat["code"]
    shared = su < 0
    u = np.where(shared, ~su, su)
    hot_i = (si & 0x80000000) != 0
    i = si & 0x7FFFFFFF
    j = rank_item[code].astype(np.int64)
    keep = ~_csr_has(indptr, indices, n_items, u, j)
    # a tile is 64 draws; its valid draws are compacted in lane order and cut into groups of UNR
    tile = cat["t"] // 64
    tile_key = (cat["phase"] * W + cat["wave"]) * (1 << 20) + tile  # (ascending in the order the draws were listed)
    assert (np.diff(tile_key) >= 0).all()
    before = np.cumsum(keep) - keep  # valid draws before this one, over the whole list
    first_of_tile = np.searchsorted(tile_key, tile_key, side="left")
    pos = before - before[first_of_tile]
    step = tile * 64 + pos // unr
    out = dict(u=u[keep], i=i[keep], j=j[keep], skipped=int((~keep).sum()), shared=shared[keep], hot_i=hot_i[keep],
               hot_j=(code < n_hot)[keep], wave=cat["wave"][keep], step=step[keep], phase=cat["phase"][keep],
               n_hot=n_hot, key=key, buckets=(sptr, rec_u, rec_i, rank_item), unr=unr, phases=(p_lo, p_hi))
    return out


def _ldsbin_mix(h):
    """murmur3 finaliser variant of csrc/bpr_ldsbin.inc ldsbin_mix on uint32 arrays."""
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x85EBCA77)) & 0xFFFFFFFF
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE3D)) & 0xFFFFFFFF
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def ldsbin_tables(indptr, indices, n_items, n_bins, hot_x1000, share=None):
    """The static tables of the LDS-bin form (csrc/bpr.hip ldsbin_build): CSC, popularity ranks, hot items and their
    interaction list in the shuffled order (stable order of a hash of the item-major list index).  share: the interaction
    count the hot threshold is a fraction of — nnz / n_bins (resident bins, the default) or nnz / (4 x CUs) (passing bins)."""
    import scipy.sparse as sp

    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    nnz, n_users = len(indices), len(indptr) - 1
    X = sp.csr_matrix((np.ones(nnz, np.int8), indices, indptr), shape=(n_users, n_items)).tocsc()
    X.sort_indices()
    cptr, cusers = X.indptr.astype(np.int32), X.indices.astype(np.int32)
    deg = np.diff(cptr)
    rank_item = np.argsort(-deg.astype(np.int64), kind="stable").astype(np.int32)
    share = nnz / n_bins if share is None else float(share)
    n_hot = 0
    while n_hot < n_items and deg[rank_item[n_hot]] * 1000.0 > share * hot_x1000:
        n_hot += 1
    hot_u = np.concatenate([cusers[cptr[i]:cptr[i + 1]] for i in rank_item[:n_hot]] + [np.zeros(0, np.int32)]).astype(np.int32)
    hot_i = np.repeat(rank_item[:n_hot], deg[rank_item[:n_hot]]).astype(np.int32)
    n_hot_inter = len(hot_u)
    if n_hot_inter:
        t = np.arange(n_hot_inter, dtype=np.uint64)
        order = np.argsort(_ldsbin_mix((t * np.uint64(0x9E3779B1) + np.uint64(0x5BD1E995)) & 0xFFFFFFFF), kind="stable")
        hot_u, hot_i = np.ascontiguousarray(hot_u[order]), np.ascontiguousarray(hot_i[order])
    else:
        hot_u = hot_i = np.zeros(1, np.int32)
    return dict(indptr=indptr, indices=indices, cptr=cptr, cusers=cusers, rank_item=rank_item, n_hot=n_hot, hot_u=hot_u,
                hot_i=hot_i, n_hot_inter=n_hot_inter, deg=deg)


def ldsbin_n_strata(n_items, n_bins, strata_groups):
    return max(1, ((n_items + n_bins - 1) // n_bins) // max(1, strata_groups))


def ldsbin_deal_key(key, n_bins, n_items, n_hot, n_strata, hot_cost_x16, rank_item, cptr, n_hot_inter):
    """One deal by its 32-bit key: (bin_of_item, cold_mass, hot_off)."""
    bin_of = np.empty(n_items, np.int32)
    cold, off = np.empty(n_bins, np.uint32), np.empty(n_bins + 1, np.uint32)
    lib().oracle_ldsbin_deal(int(key), int(n_bins), int(n_items), int(n_hot), int(n_strata), int(hot_cost_x16),
                             np.ascontiguousarray(rank_item, np.int32), np.ascontiguousarray(cptr, np.int32),
                             int(n_hot_inter), bin_of.ctypes.data, cold.ctypes.data, off.ctypes.data)
    return bin_of, cold, off


def ldsbin_deal(seed, epoch, n_bins, hot_x1000, indptr, indices, n_items, strata_groups=16, hot_cost_x16=32):
    """CPU restatement of the deal of (seed, epoch): (bin_of_item, cold_mass, hot_off, hot_u, hot_i, n_hot)."""
    t = ldsbin_tables(indptr, indices, n_items, n_bins, hot_x1000)
    key = int(lib().oracle_ldsbin_key(int(seed), int(epoch)))
    bin_of, cold, off = ldsbin_deal_key(key, n_bins, n_items, t["n_hot"], ldsbin_n_strata(n_items, n_bins, strata_groups),
                                        hot_cost_x16, t["rank_item"], t["cptr"], t["n_hot_inter"])
    return bin_of, cold, off, t["hot_u"][:t["n_hot_inter"]], t["hot_i"][:t["n_hot_inter"]], t["n_hot"]


def ldsbin_layout(deal_seed, layout_epoch, n_bins, n_items, rank_item, strata_groups=16):
    """(slot_item [n_bins cap], item_slot [n_items]) of the deal keyed by (deal_seed, layout_epoch): the order in which the
    conveyor's block buffers hold their rows (csrc/bpr_ldsbin.inc ldsbin_layout_kernel)."""
    cap = (n_items + n_bins - 1) // n_bins
    slot_item, item_slot = np.empty(n_bins * cap, np.int32), np.empty(n_items, np.int32)
    lib().oracle_ldsbin_layout(int(lib().oracle_ldsbin_key(int(deal_seed), int(layout_epoch))), int(n_bins), int(n_items),
                               int(ldsbin_n_strata(n_items, n_bins, strata_groups)), np.ascontiguousarray(rank_item, np.int32),
                               slot_item.ctypes.data, item_slot.ctypes.data)
    return slot_item, item_slot


def ldsbin_epoch(seed, epoch, n_bins, hot_x1000, indptr, indices, n_items, count_touches=False, neg_pop=False,
                 strata_groups=16, hot_cost_x16=32, tables=None, share=None, deal=None, bins=None):
    """CPU restatement of one epoch of the LDS-bin sampler (csrc/bpr_ldsbin.inc): returns (skipped, draws, n_hot[,
    positive touches per item, negative touches per item]).  deal = (deal_seed, layout_epoch): the deal's key comes from
    there instead of (seed, epoch) — the conveyor layout, whose ranks share the deal but not the draws' seed.  bins = (lo, hi): the
    draws of the bins [lo, hi) only."""
    t = tables if tables is not None else ldsbin_tables(indptr, indices, n_items, n_bins, hot_x1000, share)
    key = int(lib().oracle_ldsbin_key(int(seed), int(epoch)) if deal is None else lib().oracle_ldsbin_key(int(deal[0]), int(deal[1])))
    draws = C.c_int64()
    pos = np.zeros(n_items, np.int64) if count_touches else None
    neg = np.zeros(n_items, np.int64) if count_touches else None
    lo, hi = (0, int(n_bins)) if bins is None else (int(bins[0]), int(bins[1]))
    s = lib().oracle_ldsbin_epoch_skips_range(int(seed), int(epoch), key, int(n_bins), int(n_items), int(t["n_hot"]),
                                              int(ldsbin_n_strata(n_items, n_bins, strata_groups)), int(hot_cost_x16),
                                              t["rank_item"], t["cptr"], t["cusers"], t["hot_u"], t["hot_i"],
                                              int(t["n_hot_inter"]), t["indptr"], t["indices"], C.byref(draws),
                                              pos.ctypes.data if count_touches else None, neg.ctypes.data if count_touches else None,
                                              int(bool(neg_pop)), lo, hi)
    return (int(s), int(draws.value), t["n_hot"]) + ((pos, neg) if count_touches else ())


def hogwild_sample_owned(seed, epoch, wave_id, length, n_neg, lo, hi):
    r = np.empty(hi - lo, np.int64)
    jj = np.empty(hi - lo, np.int64)
    lib().oracle_hogwild_sample_owned(int(seed), int(epoch), int(wave_id), int(length), int(n_neg), int(lo), int(hi),
                                      r, jj)
    return r, jj


def bpr_apply_seq_f64(trip, order, U, V, B, lr, reg, use_bias):
    """float64 tables (modified in place) after the triplets' updates, one after another in `order`"""
    u, i, j = (np.ascontiguousarray(a, np.int64) for a in trip)
    order = np.ascontiguousarray(order, np.int64)
    assert U.dtype == V.dtype == B.dtype == np.float64 and len(order) <= len(u)
    lib().oracle_bpr_apply_seq_f64(u, i, j, order, len(order), U, V, B, U.shape[1], float(lr), float(reg), int(bool(use_bias)))


def bpr_jacobi_f64(trip, tables, lr, reg, use_bias):
    """every triplet's deltas from the float32 start tables, summed per row in float64: {"U" | "V" | "B": dict(sum, touches,
    path), "x", "z"} (oracle/bpr_step_oracle.py `jacobi`)"""
    u, i, j = (np.ascontiguousarray(a, np.int64) for a in trip)
    U, V, B = (np.ascontiguousarray(t, np.float32) for t in tables)
    out = {tab: dict(sum=np.zeros(t.shape), touches=np.zeros(len(t), np.int64), path=np.zeros(len(t)))
           for tab, t in (("U", U), ("V", V), ("B", B))}
    out["x"], out["z"] = np.empty(len(u)), np.empty(len(u))
    lib().oracle_bpr_jacobi_f64(u, i, j, len(u), U, V, B, U.shape[1], float(lr), float(reg), int(bool(use_bias)),
                                *[out[tab]["sum"] for tab in "UVB"], *[out[tab]["path"] for tab in "UVB"],
                                *[out[tab]["touches"] for tab in "UVB"], out["x"], out["z"])
    return out


MF_TABLES = ("U", "V", "Bu", "Bi")


def mf_apply_seq_f64(rat, order, U, V, Bu, Bi, lr, reg, mu, use_bias):
    """float64 tables (modified in place) after the ratings' updates, one after another in `order`"""
    u, i = (np.ascontiguousarray(a, np.int64) for a in rat[:2])
    r, order = np.ascontiguousarray(rat[2], np.float32), np.ascontiguousarray(order, np.int64)
    assert U.dtype == V.dtype == Bu.dtype == Bi.dtype == np.float64 and len(order) <= len(u)
    lib().oracle_mf_apply_seq_f64(u, i, r, order, len(order), U, V, Bu, Bi, U.shape[1], float(lr), float(reg), float(mu),
                                  int(bool(use_bias)))


def mf_jacobi_f64(rat, tables, lr, reg, mu, use_bias, err_floor):
    """every rating's deltas from the float32 start tables, summed per row in float64: {"U" | "V" | "Bu" | "Bi": dict(sum,
    touches, path), "err"} (oracle/mf_step_oracle.py `jacobi`)"""
    u, i = (np.ascontiguousarray(a, np.int64) for a in rat[:2])
    r = np.ascontiguousarray(rat[2], np.float32)
    tabs = [np.ascontiguousarray(t, np.float32) for t in tables]
    out = {tab: dict(sum=np.zeros(t.shape), touches=np.zeros(len(t), np.int64), path=np.zeros(len(t)))
           for tab, t in zip(MF_TABLES, tabs)}
    out["err"] = np.empty(len(u))
    lib().oracle_mf_jacobi_f64(u, i, r, len(u), *tabs, tabs[0].shape[1], float(lr), float(reg), float(mu), int(bool(use_bias)),
                               float(err_floor), *[out[tab]["sum"] for tab in MF_TABLES], *[out[tab]["path"] for tab in MF_TABLES],
                               *[out[tab]["touches"] for tab in MF_TABLES], out["err"])
    return out


def hogwild_ownership(indptr, indices, n_waves):
    """CPU restatement of the user-row ownership tables (csrc/bpr.hip build_ownership): (wave_ptr, own_u, own_i) as
    BprTrainer.debug_ownership() returns them.  Users with more than nnz / n_waves / 2 interactions are shared (own_u = ~u,
    their interactions dealt to the waves in equal blocks); the others go whole, heaviest first, to the least loaded wave."""
    import heapq

    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int32)
    nnz, W = len(indices), int(n_waves)
    deg = np.diff(indptr)
    cap = max(1, nnz // W // 2)
    n_shared = int(deg[deg > cap].sum())
    blk = (n_shared + W - 1) // W
    load = [max(0, min(blk, n_shared - w * blk)) if blk > 0 else 0 for w in range(W)]
    excl = np.flatnonzero((deg > 0) & (deg <= cap))
    excl = excl[np.argsort(-deg[excl], kind="stable")]
    heap = [(load[w], w) for w in range(W)]
    heapq.heapify(heap)
    owner = np.full(len(deg), -1, np.int64)
    for usr in excl:
        ld, w = heapq.heappop(heap)
        owner[usr] = w
        load[w] = ld + int(deg[usr])
        heapq.heappush(heap, (load[w], w))
    wave_ptr = np.concatenate([[0], np.cumsum(load)]).astype(np.int64)
    assert wave_ptr[-1] == nnz
    users = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    shared = (deg > cap)[users]
    wave = owner[users]
    wave[shared] = np.arange(n_shared) // max(blk, 1)
    # within a wave: shared positions and exclusive users interleave in user order, exactly as one pass over the users fills them
    order = np.argsort(wave, kind="stable")
    own_u = np.where(shared, ~users, users)[order].astype(np.int32)
    return wave_ptr, own_u, indices[order].astype(np.int32)


def _csr_has(indptr, indices, n_items, u, j):
    """membership of (u, j) in a CSR matrix whose rows hold sorted columns, for arrays of pairs"""
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    keys = rows * int(n_items) + np.asarray(indices, np.int64)
    q = np.asarray(u, np.int64) * int(n_items) + np.asarray(j, np.int64)
    pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return keys[pos] == q


def hogwild_triplets(form, seed, epoch, s_begin, n, indptr, indices, n_items, neg_pop=False, ownership=None, n_bins=None,
                     hot_x1000=75, share=None, strata_groups=16, hot_cost_x16=32, tables=None, deal=None, bins=None,
                     rank_item=None, k=None, hot_permille=120, hot_min_mult_x100=200, rehash_period=1):
    """The non-skipped (u, i, j) that ONE hogwild launch applies — cornac_hip_bpr_hogwild_enqueue(n) at sample offset
    s_begin of `epoch`, s_begin + n <= nnz — from the restatements of the device samplers above; integer work, exact.

      form "fused"   samples [s_begin, s_begin + n) of hogwild_sample, in sample order
      form "owned"   the tiles [own_tmax s_begin / nnz, own_tmax (s_begin + n) / nnz) of every wave's slice
                     (hogwild_sample_owned), wave by wave; ownership = BprTrainer.debug_ownership()
      form "ldsbin"  the draws [n_b s_begin / nnz, n_b (s_begin + n) / nnz) of every bin b (resident and passing bins:
                     the caller names n_bins and, for passing bins, share), bin by bin
      form "ldsbin", deal = (deal_seed, layout_epoch), bins = [(lo, hi), ...]: ONE conveyor launch —
                     cornac_hip_bpr_conveyor_enqueue(epoch, layout_epoch, blocks) — whose ranges are the bins [lo, hi) in
                     launch order (block B of bins_per_block bins: (B bpb, (B + 1) bpb)).  The deal's key comes from `deal`,
                     the draws' from (seed, epoch); no item is hot; a launch is the whole epoch of its bins (s_begin = 0,
                     n = nnz); rank_item replaces the tables' popularity order (conveyor_setup's explicit order).
      form "strata"  the XCD-strata form (csrc/bpr_strata.inc): the phases ceil(8 s_begin / nnz) up to, not including,
                     ceil(8 (s_begin + n) / nnz) (8 at the end of the epoch); in phase ph virtual wave w draws
                     len = |bucket (w, p)| times from its bucket p = ((w // 4) % 8 + ph) % 8 (strata_sample): the positive is
                     rec_u / rec_i[base + r], the negative rank_item[code].  ownership = the tables of the strata grid's
                     wave count; k picks UNR (strata_unr); hot_permille, hot_min_mult_x100, rehash_period = strata_config's.

    Returns a dict: u, i, j (int64 arrays, the restatement's order), skipped (the launch's skip count); "ldsbin" adds bin
    (the bin that drew each triplet) and hot (its positive came from the hot list); "owned" adds shared (its user is
    split over the waves: atomics on its row); "strata" adds shared, hot_i / hot_j (the item row is updated by atomics),
    wave, phase, step (tile x 64 + the triplet's group of UNR among the tile's valid draws, compacted in lane order), and
    n_hot, key, buckets (sptr, rec_u, rec_i, rank_item), unr, phases (lo, hi)."""
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    nnz, s_begin, n = len(indices), int(s_begin), int(n)
    assert 0 <= s_begin and n >= 0 and s_begin + n <= nnz
    if form == "strata":
        assert not neg_pop and ownership is not None and k is not None
        return _strata_triplets(seed, epoch, s_begin, n, indptr, indices, n_items, ownership, int(k), hot_permille,
                                hot_min_mult_x100, rehash_period)
    if form == "ldsbin":
        conveyor = deal is not None
        if conveyor:
            assert bins and s_begin == 0 and n == nnz, "a conveyor launch is the whole epoch of its ranges' bins"
            hot_x1000 = 10 ** 9
        t = tables if tables is not None else ldsbin_tables(indptr, indices, n_items, n_bins, hot_x1000, share)
        order = t["rank_item"] if rank_item is None else np.ascontiguousarray(rank_item, np.int32)
        assert not conveyor or t["n_hot"] == 0
        assert len(order) == n_items
        key = int(lib().oracle_ldsbin_key(*((int(seed), int(epoch)) if not conveyor else (int(deal[0]), int(deal[1])))))
        parts, skipped, drawn = [], 0, 0
        for lo, hi in (bins if conveyor else [(0, int(n_bins))]):
            assert 0 <= lo < hi <= n_bins
            cap = n + 2 * int(n_bins) + 8
            u, i, j, b = (np.empty(cap, np.int32) for _ in range(4))
            hot = np.empty(cap, np.uint8)
            draws, kept = C.c_int64(), C.c_int64()
            skipped += int(lib().oracle_ldsbin_draws(
                int(seed), int(epoch), key, int(n_bins), int(n_items), int(t["n_hot"]),
                int(ldsbin_n_strata(n_items, n_bins, strata_groups)), int(hot_cost_x16), order, t["cptr"], t["cusers"],
                t["hot_u"], t["hot_i"], int(t["n_hot_inter"]), t["indptr"], t["indices"], C.byref(draws), None, None,
                int(bool(neg_pop)), int(lo), int(hi), s_begin, n, nnz, u.ctypes.data, i.ctypes.data, j.ctypes.data,
                b.ctypes.data, hot.ctypes.data, cap, C.byref(kept)))
            m = int(kept.value)
            assert m <= cap
            drawn += int(draws.value)
            parts.append([a[:m] for a in (u, i, j, b, hot)])
        assert conveyor or drawn == nnz
        u, i, j, b, hot = (np.concatenate([p[q] for p in parts]) for q in range(5))
        out = dict(u=u.astype(np.int64), i=i.astype(np.int64), j=j.astype(np.int64), skipped=skipped, bin=b.astype(np.int64),
                   hot=hot.astype(bool))
        if conveyor:
            out["draws"] = drawn  # the ranges' interactions: every one is drawn (or skipped) once per epoch
        return out
    n_neg = nnz if neg_pop else int(n_items)
    if form == "fused":
        user_ids = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
        ii, jj = hogwild_sample(seed, epoch, s_begin, n, nnz, n_neg)
        u, i = user_ids[ii], indices[ii].astype(np.int64)
        shared = None
    elif form == "owned":
        wave_ptr, own_u, own_i = ownership
        lens = np.diff(wave_ptr)
        tmax = int((lens.max() + 63) // 64)
        lo_tile = tmax * s_begin // nnz
        hi_tile = tmax if s_begin + n >= nnz else tmax * (s_begin + n) // nnz
        us, is_, jjs = [], [], []
        for w in np.flatnonzero(lens > 0):
            lo, hi = min(int(lens[w]), lo_tile * 64), min(int(lens[w]), hi_tile * 64)
            if hi <= lo:
                continue
            r, jw = hogwild_sample_owned(seed, epoch, int(w), int(lens[w]), n_neg, lo, hi)
            us.append(own_u[wave_ptr[w] + r])
            is_.append(own_i[wave_ptr[w] + r])
            jjs.append(jw)
        cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
        u, i, jj = cat(us), cat(is_), cat(jjs)
        shared = u < 0
        u = np.where(shared, ~u, u)
    else:
        raise ValueError("form is 'fused', 'owned', 'ldsbin' or 'strata': %r" % (form,))
    j = indices[jj].astype(np.int64) if neg_pop else jj
    keep = ~_csr_has(indptr, indices, n_items, u, j)
    out = dict(u=u[keep], i=i[keep], j=j[keep], skipped=int((~keep).sum()))
    if shared is not None:
        out["shared"] = shared[keep]
    return out


def vebpr_hogwild_sample(seed, epoch, s0, n, n_pos, n_items):
    """unowned hogwild VEBPR sampler (csrc/vebpr.inc): (interaction index, view word, negative item) of samples [s0, s0 + n)"""
    ii, w2, jj = np.empty(n, np.int64), np.empty(n, np.uint32), np.empty(n, np.int64)
    lib().oracle_vebpr_hogwild_sample(int(seed), int(epoch), int(s0), int(n), int(n_pos), int(n_items), ii, w2, jj)
    return ii, w2, jj


def vebpr_hogwild_sample_owned(seed, epoch, wave_id, length, n_items, lo, hi):
    """owned form: (index into the wave's slice, view word, negative item) of the wave's local samples [lo, hi)"""
    r, w2, jj = np.empty(hi - lo, np.int64), np.empty(hi - lo, np.uint32), np.empty(hi - lo, np.int64)
    lib().oracle_vebpr_hogwild_sample_owned(int(seed), int(epoch), int(wave_id), int(length), int(n_items), int(lo), int(hi),
                                            r, w2, jj)
    return r, w2, jj


def hogwild_quadruples(form, seed, epoch, indptr, indices, v_indptr, v_indices, n_items, ownership=None):
    """The non-skipped (u, i, v, j) that ONE hogwild VEBPR epoch applies — cornac_hip_vebpr_fit_epochs(1, ...) is always a
    whole epoch — from the restatements of the device sampler above; integer work, exact.

      form "unowned"  samples [0, nnz) in sample order
      form "owned"    every wave's whole slice, wave by wave; ownership = (wave_ptr, own_u, own_i) as hogwild_ownership
                      restates them for the launch's wave count

    v = -1 for users without views, else v_indices[v_indptr[u] + ((w2 * nv) >> 32)].  A sample is skipped when its
    negative is in the user's purchase row or, for users with views, in the view row.  Returns a dict: u, i, v, j (int64, the
    restatement's order), draws (samples drawn), skipped (the epoch's skip count) = skipped_purchase (negative in the
    purchase row) + skipped_view_only (in the view row alone); "owned" adds shared (the user is split over the waves:
    atomics on its row)."""
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    v_indptr = np.ascontiguousarray(v_indptr, np.int64)
    v_indices = np.ascontiguousarray(v_indices, np.int32)
    nnz = len(indices)
    shared = None
    if form == "unowned":
        user_ids = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
        ii, w2, j = vebpr_hogwild_sample(seed, epoch, 0, nnz, nnz, n_items)
        u, i = user_ids[ii], indices[ii].astype(np.int64)
    elif form == "owned":
        wave_ptr, own_u, own_i = ownership
        lens = np.diff(wave_ptr)
        us, is_, ws, js = [], [], [], []
        for w in np.flatnonzero(lens > 0):
            r, w2w, jw = vebpr_hogwild_sample_owned(seed, epoch, int(w), int(lens[w]), n_items, 0, int(lens[w]))
            us.append(own_u[wave_ptr[w] + r])
            is_.append(own_i[wave_ptr[w] + r])
            ws.append(w2w)
            js.append(jw)
        u, i, j = (np.concatenate(p).astype(np.int64) for p in (us, is_, js))
        w2 = np.concatenate(ws)
        shared = u < 0
        u = np.where(shared, ~u, u)
    else:
        raise ValueError("form is 'unowned' or 'owned': %r" % (form,))
    v0 = v_indptr[u]
    nv = v_indptr[u + 1] - v0
    has_v = nv > 0
    v = np.full(len(u), -1, np.int64)
    pos = v0[has_v] + ((w2[has_v].astype(np.uint64) * nv[has_v].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    v[has_v] = v_indices[pos]
    in_purchase = _csr_has(indptr, indices, n_items, u, j)
    in_view = _csr_has(v_indptr, v_indices, n_items, u, j) if v_indptr[-1] > 0 else np.zeros(len(u), bool)
    keep = ~(in_purchase | in_view)
    out = dict(u=u[keep], i=i[keep], v=v[keep], j=j[keep], draws=len(u), skipped=int((~keep).sum()),
               skipped_purchase=int(in_purchase.sum()), skipped_view_only=int((in_view & ~in_purchase).sum()))
    if shared is not None:
        out["shared"] = shared[keep]
    return out


def vebpr_apply_seq_f64(quad, order, U, V, lr, reg, alpha, fault=0, mark=None):
    """float64 tables (modified in place) after the quadruples' hogwild VEBPR updates, one after another in `order`;
    fault = 1 + its index in vebpr_step_oracle.FAULTS; mark = (table "U" | "V", row, sign): that row's last update is
    applied once more with that factor"""
    u, i, v, j = (np.ascontiguousarray(a, np.int64) for a in quad)
    order = np.ascontiguousarray(order, np.int64)
    assert U.dtype == V.dtype == np.float64 and U.flags.c_contiguous and V.flags.c_contiguous and len(order) <= len(u)
    tab, row, sign = (0, 0, 0.0) if mark is None else ({"U": 1, "V": 2}[mark[0]], int(mark[1]), float(mark[2]))
    lib().oracle_vebpr_apply_seq_f64(u, i, v, j, order, len(order), U, V, U.shape[1], float(lr), float(reg), float(alpha),
                                     int(fault), tab, row, sign)


def vebpr_jacobi_f64(quad, tables, lr, reg, alpha):
    """every quadruple's deltas from the float32 start tables, summed per row in float64: {"U" | "V": dict(sum, touches,
    path), "x": [n, 3] clamped scores x_ij, x_iv, x_vj} (oracle/vebpr_step_oracle.py `jacobi`)"""
    u, i, v, j = (np.ascontiguousarray(a, np.int64) for a in quad)
    U, V = (np.ascontiguousarray(t, np.float32) for t in tables[:2])
    out = {tab: dict(sum=np.zeros(t.shape), touches=np.zeros(len(t), np.int64), path=np.zeros(len(t)))
           for tab, t in (("U", U), ("V", V))}
    out["x"] = np.zeros((len(u), 3))
    lib().oracle_vebpr_jacobi_f64(u, i, v, j, len(u), U, V, U.shape[1], float(lr), float(reg), float(alpha),
                                  *[out[tab]["sum"] for tab in "UV"], *[out[tab]["path"] for tab in "UV"],
                                  *[out[tab]["touches"] for tab in "UV"], out["x"])
    return out

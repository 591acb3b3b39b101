"""ctypes binding of libcornac_hip.so (the C ABI declared in include/cornac_hip.h).

There is deliberately NO fallback: if the shared library is missing, or no
gfx950 device is visible when a kernel is requested, the product path raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CORNAC_HIP_PROFILE=1 loads the -DCORNAC_PROFILE build of the same sources (A/B switches and ablation bits compiled
# in; `make -C cornac_amd/csrc PROFILE=1`): tools/ only — the tests, bench.py and smoke() use the shipped library
PROFILE = os.environ.get("CORNAC_HIP_PROFILE", "") == "1"
LIB_PATH = os.path.join(_HERE, "lib", "libcornac_hip_profile.so" if PROFILE else "libcornac_hip.so")
CSRC = os.path.join(_HERE, "csrc")

MODE_DETERMINISTIC = 0
MODE_HOGWILD = 1
VEBPR_NO_OWNERSHIP = 0x100
# hogwild_flags (include/cornac_hip.h, CORNAC_HIP_HOG_* / CORNAC_HIP_FORM_*): the form field of a hogwild call ...
HOG_FORM_MASK, HOG_FORM_SHIFT = 0xF0000, 16
FORM_AUTO, FORM_FUSED, FORM_STRATA, FORM_LDSBIN = (f << HOG_FORM_SHIFT for f in range(4))
# ... the switches below it (bit 5, value 32, is reserved) and the ablation field of the profile build
HOG_PLAIN_STORES, HOG_VEC4_LAYOUT, HOG_NO_OWNERSHIP, HOG_DENSE_BIAS, HOG_SHARE_NEG = 1, 2, 4, 8, 16
HOG_BINNED, HOG_FUSED_OPT_OUT = 64, 128
HOG_ABLATE_MASK, HOG_ABLATE_SHIFT = 0xFF00, 8
NEG_UNIFORM = 0
NEG_POPULARITY = 1

# every symbol include/cornac_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "cornac_hip_last_error", "cornac_hip_version", "cornac_hip_device_count", "cornac_hip_device_info",
    "cornac_hip_device_probe",
    "cornac_hip_bpr_create", "cornac_hip_bpr_destroy", "cornac_hip_bpr_set_factors", "cornac_hip_bpr_get_factors",
    "cornac_hip_bpr_bind_device", "cornac_hip_bpr_rebind_items", "cornac_hip_bpr_conveyor_setup", "cornac_hip_bpr_conveyor_layout", "cornac_hip_bpr_conveyor_enqueue", "cornac_hip_bpr_set_negative_population", "cornac_hip_bpr_device_ptrs", "cornac_hip_bpr_set_stream",
    "cornac_hip_bpr_seed_mt19937", "cornac_hip_bpr_seed_hogwild", "cornac_hip_bpr_fit_epochs",
    "cornac_hip_bpr_set_factors_f64", "cornac_hip_bpr_get_factors_f64", "cornac_hip_bpr_fit_epochs_f64",
    "cornac_hip_bpr_hogwild_enqueue", "cornac_hip_bpr_sync", "cornac_hip_bpr_debug_draw",
    "cornac_hip_bpr_last_timing", "cornac_hip_bpr_kernel_timing", "cornac_hip_mf_kernel_timing",
    "cornac_hip_bpr_debug_ownership", "cornac_hip_bpr_set_views", "cornac_hip_bpr_seed_view_stream",
    "cornac_hip_vebpr_fit_epochs", "cornac_hip_vebpr_fit_epochs_f64", "cornac_hip_vebpr_hogwild_form",
    "cornac_hip_mmmf_fit_epochs", "cornac_hip_mmmf_fit_epochs_f64", "cornac_hip_mmmf_hogwild_enqueue",
    "cornac_hip_bpr_strata_config", "cornac_hip_bpr_chunk_records", "cornac_hip_bpr_strata_stats", "cornac_hip_bpr_debug_strata",
    "cornac_hip_bpr_ldsbin_config", "cornac_hip_bpr_ldsbin_pass_config", "cornac_hip_bpr_ldsbin_stats",
    "cornac_hip_bpr_ldsbin_deal_config", "cornac_hip_bpr_debug_ldsbin_deal",
    "cornac_hip_bpr_sample_triplets", "cornac_hip_bpr_apply_triplets", "cornac_hip_bpr_gather_rows",
    "cornac_hip_bpr_staged_slots", "cornac_hip_bpr_emit_triplets", "cornac_hip_bpr_apply_staged",
    "cornac_hip_bpr_shard_mark", "cornac_hip_bpr_shard_slots", "cornac_hip_bpr_shard_uniq",
    "cornac_hip_bpr_scatter_diff_rows", "cornac_hip_bpr_switch_stream",
    "cornac_hip_bpr_scatter_add_rows", "cornac_hip_bpr_table_delta_begin", "cornac_hip_bpr_table_delta_finish",
    "cornac_hip_bpr_table_delta_step", "cornac_hip_table_delta", "cornac_hip_bpr_table_delta",
    "cornac_hip_bpr_resident_exchange_bins", "cornac_hip_bpr_epoch_resident_enqueue", "cornac_hip_bpr_resident_flush",
    "cornac_hip_stream_wait_counter", "cornac_hip_stream_set_flag", "cornac_hip_stream_ring_standin",
    "cornac_hip_vbpr_create", "cornac_hip_vbpr_destroy", "cornac_hip_vbpr_set_params", "cornac_hip_vbpr_get_params",
    "cornac_hip_vbpr_fit_batches", "cornac_hip_vbpr_item_tables",
    "cornac_hip_wmf_create", "cornac_hip_wmf_destroy", "cornac_hip_wmf_set_factors", "cornac_hip_wmf_get_factors",
    "cornac_hip_wmf_fit_batches", "cornac_hip_wmf_kernel_timing", "cornac_hip_wmf_last_timing",
    "cornac_hip_mf_create", "cornac_hip_mf_destroy", "cornac_hip_mf_set_factors", "cornac_hip_mf_get_factors",
    "cornac_hip_mf_fit", "cornac_hip_mf_bind_items", "cornac_hip_mf_bind_users", "cornac_hip_mf_set_stream", "cornac_hip_mf_epoch_enqueue",
    "cornac_hip_mf_sync", "cornac_hip_mf_fit_sgd", "cornac_hip_mf_last_timing", "cornac_hip_mf_det_form",
    "cornac_hip_mf_hogwild_form", "cornac_hip_mf_hogwild_stats", "cornac_hip_mf_debug_split", "cornac_hip_mf_debug_ownership",
    "cornac_hip_mf_fit_minibatch", "cornac_hip_mf_fit_minibatch_dropout", "cornac_hip_mf_reset_optimizer",
    "cornac_hip_mf_pmf_set_factors", "cornac_hip_mf_pmf_get_factors", "cornac_hip_mf_pmf_fit", "cornac_hip_mf_pmf_form",
    "cornac_hip_mf_nmf_set_factors", "cornac_hip_mf_nmf_get_factors", "cornac_hip_mf_nmf_fit", "cornac_hip_mf_nmf_form",
    "cornac_hip_mf_hpf_set_tables", "cornac_hip_mf_hpf_get_tables", "cornac_hip_mf_hpf_fit", "cornac_hip_mf_hpf_elog",
    "cornac_hip_mf_hpf_form",
    "cornac_hip_scorer_create", "cornac_hip_scorer_destroy", "cornac_hip_scorer_set", "cornac_hip_score_user",
    "cornac_hip_scorer_set_f64", "cornac_hip_score_user_f64",
    "cornac_hip_score_block", "cornac_hip_rank_topk", "cornac_hip_rank_topk_device", "cornac_hip_score_pairs",
    "cornac_hip_scorer_set_exclusions", "cornac_hip_rank_topk_resident", "cornac_hip_scorer_host_buffer",
    "cornac_hip_rank_positions",
    "cornac_hip_knn_sim_create", "cornac_hip_knn_sim_destroy", "cornac_hip_knn_sim_run", "cornac_hip_knn_sim_nnz",
    "cornac_hip_knn_sim_get",
    "cornac_hip_knn_scorer_create", "cornac_hip_knn_scorer_destroy", "cornac_hip_knn_scorer_score_users",
    "cornac_hip_knn_scorer_score_pairs",
    "cornac_hip_ease_create", "cornac_hip_ease_destroy", "cornac_hip_ease_gram", "cornac_hip_ease_invert",
    "cornac_hip_ease_weights", "cornac_hip_ease_fit", "cornac_hip_ease_get_table", "cornac_hip_ease_set_table",
    "cornac_hip_ease_score_users", "cornac_hip_ease_score_pairs",
    "cornac_hip_vaecf_create", "cornac_hip_vaecf_destroy", "cornac_hip_vaecf_set_params", "cornac_hip_vaecf_get_params",
    "cornac_hip_vaecf_get_state", "cornac_hip_vaecf_reset_optimizer", "cornac_hip_vaecf_fit_epoch",
    "cornac_hip_vaecf_encode_users", "cornac_hip_vaecf_score_users", "cornac_hip_vaecf_score_pairs",
    "cornac_hip_bivae_create", "cornac_hip_bivae_destroy", "cornac_hip_bivae_set_params", "cornac_hip_bivae_get_params",
    "cornac_hip_bivae_set_factors", "cornac_hip_bivae_get_factors", "cornac_hip_bivae_get_state",
    "cornac_hip_bivae_reset_optimizer", "cornac_hip_bivae_fit_epoch", "cornac_hip_bivae_last_timing",
    "cornac_hip_bivae_infer_means",
    "cornac_hip_bivae_score_users", "cornac_hip_bivae_score_pairs",
    "cornac_hip_ncf_create", "cornac_hip_ncf_destroy", "cornac_hip_ncf_n_tables", "cornac_hip_ncf_set_params",
    "cornac_hip_ncf_get_params", "cornac_hip_ncf_get_state", "cornac_hip_ncf_reset_optimizer", "cornac_hip_ncf_fit_epoch",
    "cornac_hip_ncf_draw_epoch", "cornac_hip_ncf_fit_epoch_sampled", "cornac_hip_ncf_score_users", "cornac_hip_ncf_score_pairs",
    "cornac_hip_lightgcn_create", "cornac_hip_lightgcn_destroy", "cornac_hip_lightgcn_set_params", "cornac_hip_lightgcn_get_params",
    "cornac_hip_lightgcn_get_state", "cornac_hip_lightgcn_reset_optimizer", "cornac_hip_lightgcn_fit_epoch",
    "cornac_hip_lightgcn_propagate",
    "cornac_hip_ngcf_create", "cornac_hip_ngcf_destroy", "cornac_hip_ngcf_set_params", "cornac_hip_ngcf_get_params",
    "cornac_hip_ngcf_get_state", "cornac_hip_ngcf_reset_optimizer", "cornac_hip_ngcf_fit_epoch", "cornac_hip_ngcf_propagate",
    "cornac_hip_recvae_create", "cornac_hip_recvae_destroy", "cornac_hip_recvae_set_params", "cornac_hip_recvae_get_params",
    "cornac_hip_recvae_get_state", "cornac_hip_recvae_reset_optimizer", "cornac_hip_recvae_update_prior",
    "cornac_hip_recvae_get_prior_posterior", "cornac_hip_recvae_fit_epoch", "cornac_hip_recvae_encode_users",
    "cornac_hip_recvae_score_users", "cornac_hip_recvae_score_pairs",
]


class HipError(RuntimeError):
    """A libcornac_hip call returned a non-zero status."""

    def __init__(self, code, msg):
        super().__init__("libcornac_hip error %d: %s" % (code, msg))
        self.code = code


def build(force=False, verbose=False):
    """Compile libcornac_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j", "4"] + (["-B"] if force else []) + (["PROFILE=1"] if PROFILE else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise RuntimeError("building libcornac_hip.so failed")
    return LIB_PATH


_lib = None

_f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64 = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_vp = C.c_void_p


def _preload_torch_hip_runtime():
    """One process must use ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so; if
    torch is imported after this library has pulled in /opt/rocm's copy, torch finds no GPUs (and the other
    way round works).  So when a torch wheel with a bundled runtime is installed, load that copy first
    (by path, without importing torch); the multi-GPU driver (torch.distributed + this library in one
    process) then shares it."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    except Exception:
        return
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    """Load the shared library (raises if it has not been built — no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libcornac_hip.so not found at %s. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C cornac_amd/csrc`. cornac_amd has no CPU fallback." % LIB_PATH)
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.cornac_hip_last_error.restype = C.c_char_p
        L.cornac_hip_version.restype = C.c_char_p
        L.cornac_hip_device_count.argtypes = [C.POINTER(C.c_int)]
        L.cornac_hip_device_info.argtypes = [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        L.cornac_hip_device_probe.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_double)]
        L.cornac_hip_bpr_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_int, _i32, _i32, C.c_int64]
        L.cornac_hip_bpr_destroy.argtypes = [_vp]
        L.cornac_hip_bpr_set_factors.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_get_factors.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_bind_device.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_rebind_items.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_bpr_conveyor_setup.argtypes = [_vp, C.c_int, _vp, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int)]
        L.cornac_hip_bpr_conveyor_layout.argtypes = [_vp, C.c_uint32, _vp, _vp]
        L.cornac_hip_bpr_conveyor_enqueue.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int32), C.POINTER(_vp),
                                                      C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        L.cornac_hip_bpr_set_negative_population.argtypes = [_vp, _vp, C.c_int64]
        L.cornac_hip_bpr_device_ptrs.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]
        L.cornac_hip_bpr_set_stream.argtypes = [_vp, _vp]
        L.cornac_hip_bpr_switch_stream.argtypes = [_vp, _vp]
        L.cornac_hip_bpr_seed_mt19937.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_int]
        L.cornac_hip_bpr_seed_hogwild.argtypes = [_vp, C.c_uint64]
        L.cornac_hip_bpr_fit_epochs.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_set_factors_f64.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_get_factors_f64.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_fit_epochs_f64.argtypes = [_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_hogwild_enqueue.argtypes = [_vp, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        L.cornac_hip_bpr_sync.argtypes = [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_debug_draw.argtypes = [_vp, C.c_int, C.c_uint64, C.c_int64, _i64]
        L.cornac_hip_bpr_last_timing.argtypes = [_vp, C.POINTER(C.c_double)]
        L.cornac_hip_bpr_set_views.argtypes = [_vp, _i32, _i32, C.c_int64]
        L.cornac_hip_bpr_seed_view_stream.argtypes = [_vp, C.c_uint32]
        L.cornac_hip_vebpr_hogwild_form.argtypes = [_vp, C.POINTER(C.c_int)]
        L.cornac_hip_vebpr_fit_epochs.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int,
                                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_vebpr_fit_epochs_f64.argtypes = [_vp, C.c_int, C.c_double, C.c_double, C.c_double,
                                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_mmmf_fit_epochs.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64)]
        L.cornac_hip_mmmf_fit_epochs_f64.argtypes = [_vp, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int64),
                                                     C.POINTER(C.c_int64)]
        L.cornac_hip_mmmf_hogwild_enqueue.argtypes = [_vp, C.c_int64, C.c_float, C.c_float]
        L.cornac_hip_bpr_sample_triplets.argtypes = [_vp, C.c_int64, C.c_int, _vp, _vp, _vp]
        L.cornac_hip_bpr_apply_triplets.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int, C.c_float,
                                                    C.c_float, C.c_int]
        L.cornac_hip_bpr_gather_rows.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, _vp]
        L.cornac_hip_bpr_staged_slots.argtypes = [_vp, C.c_int64, C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_emit_triplets.argtypes = [_vp, C.c_int64, C.c_int, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_apply_staged.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int, C.c_float, C.c_float,
                                                  C.c_int]
        L.cornac_hip_bpr_shard_mark.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp]
        L.cornac_hip_bpr_shard_slots.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int64, _vp, _vp, _vp]
        L.cornac_hip_bpr_shard_uniq.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int64, _vp]
        L.cornac_hip_bpr_scatter_diff_rows.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]
        L.cornac_hip_bpr_scatter_add_rows.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, _vp]
        L.cornac_hip_bpr_table_delta_begin.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp]
        L.cornac_hip_bpr_table_delta_finish.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int]
        L.cornac_hip_bpr_table_delta_step.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp]
        L.cornac_hip_table_delta.argtypes = [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp]
        L.cornac_hip_bpr_table_delta.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp]
        L.cornac_hip_bpr_resident_exchange_bins.argtypes = [_vp, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.cornac_hip_bpr_epoch_resident_enqueue.argtypes = [_vp, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                                            C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp,
                                                            C.POINTER(C.c_int)]
        L.cornac_hip_bpr_resident_flush.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp]
        L.cornac_hip_stream_wait_counter.argtypes = [C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_int]
        L.cornac_hip_stream_set_flag.argtypes = [C.c_int, _vp, _vp, C.c_uint32, _vp]
        L.cornac_hip_stream_ring_standin.argtypes = [C.c_int, _vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int64, C.c_int]
        L.cornac_hip_bpr_debug_ownership.argtypes = [_vp, C.POINTER(C.c_int64), _vp, _vp, _vp]
        L.cornac_hip_bpr_strata_config.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
        L.cornac_hip_bpr_chunk_records.argtypes = [_vp, C.c_int]
        L.cornac_hip_bpr_strata_stats.argtypes = [_vp, C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_debug_strata.argtypes = [_vp, C.c_uint32, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint32)]
        L.cornac_hip_bpr_ldsbin_config.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
        L.cornac_hip_bpr_ldsbin_pass_config.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cornac_hip_bpr_ldsbin_stats.argtypes = [_vp, C.POINTER(C.c_int64)]
        L.cornac_hip_bpr_ldsbin_deal_config.argtypes = [_vp, C.c_int, C.c_int]
        L.cornac_hip_bpr_debug_ldsbin_deal.argtypes = [_vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_bpr_kernel_timing.argtypes = [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.cornac_hip_mf_kernel_timing.argtypes = [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.cornac_hip_vbpr_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _f32]
        L.cornac_hip_vbpr_destroy.argtypes = [_vp]
        L.cornac_hip_vbpr_set_params.argtypes = [_vp] + [_vp] * 6
        L.cornac_hip_vbpr_get_params.argtypes = [_vp] + [_vp] * 6
        L.cornac_hip_vbpr_fit_batches.argtypes = [_vp, _i32, _i32, _i32, C.c_int64, C.c_int, C.c_float, C.c_float,
                                                  C.c_float, C.c_float, C.POINTER(C.c_double)]
        L.cornac_hip_vbpr_item_tables.argtypes = [_vp, _f32, _f32]
        L.cornac_hip_mf_fit_minibatch.argtypes = [_vp, _i64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float,
                                                  C.c_float, C.c_int, C.POINTER(C.c_double)]
        L.cornac_hip_mf_fit_minibatch_dropout.argtypes = [_vp, _i64, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float,
                                                          C.c_float, C.c_int, _vp, _vp, C.c_float, C.POINTER(C.c_double)]
        L.cornac_hip_mf_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_mf_pmf_set_factors.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_mf_pmf_get_factors.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_mf_pmf_fit.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, _vp]
        L.cornac_hip_mf_pmf_form.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cornac_hip_mf_det_form.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cornac_hip_mf_nmf_set_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_mf_nmf_get_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_mf_nmf_fit.argtypes = [_vp, C.c_int] + [C.c_float] * 6 + [C.c_int, C.c_int, _vp]
        L.cornac_hip_mf_nmf_form.argtypes = [_vp] + [C.POINTER(C.c_int)] * 3
        L.cornac_hip_mf_hpf_set_tables.argtypes = [_vp] * 5
        L.cornac_hip_mf_hpf_get_tables.argtypes = [_vp] * 7
        L.cornac_hip_mf_hpf_fit.argtypes = [_vp, C.c_int, C.c_int]
        L.cornac_hip_mf_hpf_elog.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_mf_hpf_form.argtypes = [_vp] + [C.POINTER(C.c_int)] * 2
        L.cornac_hip_wmf_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int, _i64, _i32, _f32,
                                            C.c_int64]
        L.cornac_hip_wmf_destroy.argtypes = [_vp]
        L.cornac_hip_wmf_destroy.restype = None
        L.cornac_hip_wmf_set_factors.argtypes = [_vp, _f32, _f32]
        L.cornac_hip_wmf_get_factors.argtypes = [_vp, _f32, _f32]
        L.cornac_hip_wmf_fit_batches.argtypes = [_vp, _i32, _i64, C.c_int64, C.c_float, C.c_float, C.c_float,
                                                 C.c_float, C.c_float, _vp]
        L.cornac_hip_wmf_kernel_timing.argtypes = [_vp, C.c_int]
        L.cornac_hip_wmf_last_timing.argtypes = [_vp, C.POINTER(C.c_double)]
        L.cornac_hip_mf_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int, _i64, _i64, _f32,
                                           C.c_int64]
        L.cornac_hip_mf_destroy.argtypes = [_vp]
        L.cornac_hip_mf_set_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_mf_get_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_mf_bind_items.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_mf_bind_users.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_mf_set_stream.argtypes = [_vp, _vp]
        L.cornac_hip_mf_epoch_enqueue.argtypes = [_vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
        L.cornac_hip_mf_sync.argtypes = [_vp, C.POINTER(C.c_double)]
        L.cornac_hip_mf_fit.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, _vp,
                                        C.POINTER(C.c_int)]
        L.cornac_hip_mf_fit_sgd.argtypes = [C.c_int, _i64, _i64, _f32, C.c_int64, _f32, _f32, _f32, _f32, C.c_int64,
                                            C.c_int64, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                            C.c_int, C.c_int, _vp, C.POINTER(C.c_int)]
        L.cornac_hip_mf_last_timing.argtypes = [_vp, C.POINTER(C.c_double)]
        L.cornac_hip_mf_hogwild_form.argtypes = [_vp, C.c_int]
        L.cornac_hip_mf_hogwild_stats.argtypes = [_vp, C.POINTER(C.c_int64)]
        L.cornac_hip_mf_debug_split.argtypes = [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp, _vp]
        L.cornac_hip_mf_debug_ownership.argtypes = [_vp, C.POINTER(C.c_int64), _vp, _vp, _vp]
        L.cornac_hip_scorer_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int]
        L.cornac_hip_scorer_destroy.argtypes = [_vp]
        L.cornac_hip_scorer_set.argtypes = [_vp, _f32, _f32, _vp, _vp]
        L.cornac_hip_score_user.argtypes = [_vp, C.c_int64, _f32]
        L.cornac_hip_scorer_set_f64.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_score_user_f64.argtypes = [_vp, C.c_int64, _vp]
        L.cornac_hip_score_block.argtypes = [_vp, _i32, C.c_int64, _f32]
        L.cornac_hip_score_pairs.argtypes = [_vp, _i32, _i32, C.c_int64, C.c_int, C.c_float, C.c_float, _f32]
        L.cornac_hip_rank_topk.argtypes = [_vp, _i32, C.c_int64, C.c_int, _vp, _vp, _i32, _f32]
        L.cornac_hip_rank_positions.argtypes = [_vp, _i32, C.c_int64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32]
        L.cornac_hip_rank_topk_device.argtypes = [_vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.cornac_hip_scorer_set_exclusions.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_scorer_host_buffer.argtypes = [_vp, C.c_size_t, C.POINTER(_vp)]
        L.cornac_hip_rank_topk_resident.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int, _vp, _vp, _vp]
        L.cornac_hip_knn_sim_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp]
        L.cornac_hip_knn_sim_destroy.argtypes = [_vp]
        L.cornac_hip_knn_sim_run.argtypes = [_vp, C.c_int64]
        L.cornac_hip_knn_sim_nnz.argtypes = [_vp, C.POINTER(C.c_int64)]
        L.cornac_hip_knn_sim_get.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_knn_scorer_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, C.c_int64] + [_vp] * 6 + [C.c_int]
        L.cornac_hip_knn_scorer_destroy.argtypes = [_vp]
        L.cornac_hip_knn_scorer_score_users.argtypes = [_vp, _vp, C.c_int64, C.c_int, _vp]
        L.cornac_hip_knn_scorer_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, _vp]
        L.cornac_hip_ease_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp]
        L.cornac_hip_ease_destroy.argtypes = [_vp]
        L.cornac_hip_ease_gram.argtypes = [_vp]
        L.cornac_hip_ease_invert.argtypes = [_vp, C.c_double]
        L.cornac_hip_ease_weights.argtypes = [_vp, C.c_int]
        L.cornac_hip_ease_fit.argtypes = [_vp, C.c_double, C.c_int]
        L.cornac_hip_ease_get_table.argtypes = [_vp, _vp]
        L.cornac_hip_ease_set_table.argtypes = [_vp, _vp]
        L.cornac_hip_ease_score_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_ease_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
        L.cornac_hip_vaecf_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                              C.c_int]
        L.cornac_hip_vaecf_destroy.argtypes = [_vp]
        L.cornac_hip_vaecf_set_params.argtypes = [_vp, _vp]
        L.cornac_hip_vaecf_get_params.argtypes = [_vp, _vp]
        L.cornac_hip_vaecf_get_state.argtypes = [_vp, _vp, _vp, C.POINTER(C.c_int64)]
        L.cornac_hip_vaecf_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_vaecf_fit_epoch.argtypes = [_vp, C.c_int64, C.c_float, C.c_float, _vp, C.c_uint64, C.POINTER(C.c_double), _vp]
        L.cornac_hip_vaecf_encode_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_vaecf_score_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_vaecf_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
        L.cornac_hip_bivae_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                              C.c_int]
        L.cornac_hip_bivae_destroy.argtypes = [_vp]
        L.cornac_hip_bivae_set_params.argtypes = [_vp, _vp]
        L.cornac_hip_bivae_get_params.argtypes = [_vp, _vp]
        L.cornac_hip_bivae_set_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_bivae_get_factors.argtypes = [_vp, _vp, _vp, _vp, _vp]
        L.cornac_hip_bivae_get_state.argtypes = [_vp, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_bivae_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_bivae_fit_epoch.argtypes = [_vp, C.c_int64, C.c_float, C.c_float, _vp, _vp, C.c_uint64, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), _vp]
        L.cornac_hip_bivae_last_timing.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.cornac_hip_bivae_infer_means.argtypes = [_vp]
        L.cornac_hip_bivae_score_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_bivae_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
        L.cornac_hip_ncf_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, _vp, C.c_int,
                                            C.c_int]
        L.cornac_hip_ncf_destroy.argtypes = [_vp]
        L.cornac_hip_ncf_n_tables.argtypes = [_vp, C.POINTER(C.c_int)]
        L.cornac_hip_ncf_set_params.argtypes = [_vp, _vp]
        L.cornac_hip_ncf_get_params.argtypes = [_vp, _vp]
        L.cornac_hip_ncf_get_state.argtypes = [_vp, _vp, _vp, C.POINTER(C.c_int64)]
        L.cornac_hip_ncf_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_ncf_fit_epoch.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_double), _vp]
        L.cornac_hip_ncf_draw_epoch.argtypes = [_vp, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp]
        L.cornac_hip_ncf_fit_epoch_sampled.argtypes = [_vp, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_int,
                                                       C.POINTER(C.c_double), _vp]
        L.cornac_hip_ncf_score_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_ncf_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
        L.cornac_hip_lightgcn_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int, C.c_int]
        L.cornac_hip_lightgcn_destroy.argtypes = [_vp]
        L.cornac_hip_lightgcn_set_params.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_lightgcn_get_params.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_lightgcn_get_state.argtypes = [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int64)]
        L.cornac_hip_lightgcn_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_lightgcn_fit_epoch.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp]
        L.cornac_hip_lightgcn_propagate.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_ngcf_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_uint64]
        L.cornac_hip_ngcf_destroy.argtypes = [_vp]
        L.cornac_hip_ngcf_set_params.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_ngcf_get_params.argtypes = [_vp, _vp, _vp, _vp]
        L.cornac_hip_ngcf_get_state.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int64)]
        L.cornac_hip_ngcf_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_ngcf_fit_epoch.argtypes = [_vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp]
        L.cornac_hip_ngcf_propagate.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_recvae_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int, C.c_int]
        L.cornac_hip_recvae_destroy.argtypes = [_vp]
        L.cornac_hip_recvae_set_params.argtypes = [_vp, _vp]
        L.cornac_hip_recvae_get_params.argtypes = [_vp, _vp]
        L.cornac_hip_recvae_get_state.argtypes = [_vp, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.cornac_hip_recvae_reset_optimizer.argtypes = [_vp]
        L.cornac_hip_recvae_update_prior.argtypes = [_vp]
        L.cornac_hip_recvae_get_prior_posterior.argtypes = [_vp, _vp, _vp]
        L.cornac_hip_recvae_fit_epoch.argtypes = [_vp, _vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                                  _vp, _vp, C.c_uint64, _vp]
        L.cornac_hip_recvae_encode_users.argtypes = [_vp, _vp, C.c_int64, _vp, _vp]
        L.cornac_hip_recvae_score_users.argtypes = [_vp, _vp, C.c_int64, _vp]
        L.cornac_hip_recvae_score_pairs.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise HipError(rc, lib().cornac_hip_last_error().decode("utf-8", "replace"))


def stream_wait_counter(device, stream, d_counter, target, d_error, timeout_ms=5000):
    """enqueue on `stream` (a hipStream_t as int): wait until *d_counter >= target; after timeout_ms *d_error = 1"""
    check(lib().cornac_hip_stream_wait_counter(int(device), stream, d_counter, int(target), d_error, int(timeout_ms)))


def stream_ring_standin(device, stream, d_src, src_floats, d_dst, dst_floats, n_floats, n_workgroups=16):
    """what a ring all-reduce would move through this rank, as n_workgroups workgroups on `stream` (measurement aid)"""
    check(lib().cornac_hip_stream_ring_standin(int(device), stream, d_src, int(src_floats), d_dst, int(dst_floats),
                                               int(n_floats), int(n_workgroups)))


def stream_set_flag(device, stream, d_flag, value=1, d_unless=None):
    """*d_flag = value on `stream` — unless d_unless is given and *d_unless != 0 (an earlier stream_wait_counter gave up)"""
    check(lib().cornac_hip_stream_set_flag(int(device), stream, d_flag, int(value), d_unless))


def device_count():
    n = C.c_int(0)
    check(lib().cornac_hip_device_count(C.byref(n)))
    return n.value


def device_probe(device=0, nbytes=6 << 30):
    """memory-system calibration of this box: GB/s of a device-to-device copy, a streaming read and random 512-byte
    row gathers over buffers of nbytes"""
    o = (C.c_double * 3)()
    check(lib().cornac_hip_device_probe(device, int(nbytes), o))
    return {"d2d_copy_GBps": o[0], "stream_read_GBps": o[1], "row_gather_512B_GBps": o[2], "buffer_bytes": int(nbytes)}


def device_info(device=0):
    name = C.create_string_buffer(256)
    cus = C.c_int()
    mem = C.c_int64()
    check(lib().cornac_hip_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": mem.value}


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f32c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class _HandleOwner:
    """Owner of one native handle, kept in the attribute `_HANDLE` names and released by the library's `_DESTROY`.  close()
    may be called twice, after an __init__ that failed before the handle existed, and while the interpreter shuts down."""
    _DESTROY = None
    _HANDLE = "h"

    def close(self):
        h = getattr(self, self._HANDLE, None)
        if h is not None and h and lib is not None:
            getattr(lib(), self._DESTROY)(h)
            setattr(self, self._HANDLE, None)

    __del__ = close


def _score_by_ids(symbol, h, dtype, users, items=None, width=None, extra=()):
    """`symbol`(h, users[, items], n, *extra, out) over contiguous int32 ids: out is [n, width] (a row per user) or, for
    pairs, [n]"""
    ids = [np.ascontiguousarray(users, np.int32)] + ([] if items is None else [np.ascontiguousarray(items, np.int32)])
    n = len(ids[0])
    assert all(len(a) == n for a in ids)
    out = np.empty(n if width is None else (n, width), dtype)
    check(getattr(lib(), symbol)(h, *[_ptr(a) for a in ids], n, *extra, _ptr(out)))
    return out


class BprTrainer(_HandleOwner):
    """Thin owner of a cornac_hip_bpr_t handle."""
    _DESTROY = "cornac_hip_bpr_destroy"

    def __init__(self, indptr, indices, n_users, n_items, total_users, total_items, k, device=0):
        self.indptr = np.ascontiguousarray(indptr, np.int32)
        self.indices = np.ascontiguousarray(indices, np.int32)
        self.shape = (int(total_users), int(total_items), int(k))
        self.nnz = len(self.indices)
        self.n_items = int(n_items)
        self.device, self._stream = int(device), None
        self.h = _vp()
        check(lib().cornac_hip_bpr_create(C.byref(self.h), device, n_users, n_items, total_users, total_items, k,
                                          self.indptr, self.indices, self.nnz))

    def set_factors(self, U=None, V=None, B=None):
        U, V, B = _f32c(U), _f32c(V), _f32c(B)
        tu, ti, k = self.shape
        assert U is None or U.shape == (tu, k)
        assert V is None or V.shape == (ti, k)
        assert B is None or B.shape == (ti,)
        check(lib().cornac_hip_bpr_set_factors(self.h, _ptr(U), _ptr(V), _ptr(B)))

    def get_factors(self):
        tu, ti, k = self.shape
        U, V, B = np.empty((tu, k), np.float32), np.empty((ti, k), np.float32), np.empty(ti, np.float32)
        check(lib().cornac_hip_bpr_get_factors(self.h, U.ctypes.data, V.ctypes.data, B.ctypes.data))
        return U, V, B

    def set_factors_f64(self, U, V, B):
        """float64 tables (recom_bpr.pyx:211-214 is a fused-type function): the handle then trains in double"""
        tu, ti, k = self.shape
        U, V, B = (np.ascontiguousarray(a, np.float64) for a in (U, V, B))
        assert U.shape == (tu, k) and V.shape == (ti, k) and B.shape == (ti,)
        check(lib().cornac_hip_bpr_set_factors_f64(self.h, U.ctypes.data, V.ctypes.data, B.ctypes.data))

    def get_factors_f64(self):
        tu, ti, k = self.shape
        U, V, B = np.empty((tu, k), np.float64), np.empty((ti, k), np.float64), np.empty(ti, np.float64)
        check(lib().cornac_hip_bpr_get_factors_f64(self.h, U.ctypes.data, V.ctypes.data, B.ctypes.data))
        return U, V, B

    def fit_epochs_f64(self, n_epochs, lr, reg, use_bias=True, neg_population=NEG_UNIFORM):
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_bpr_fit_epochs_f64(self.h, n_epochs, float(lr), float(reg), int(use_bias), neg_population,
                                                  C.byref(c), C.byref(s)))
        return c.value, s.value

    def get_user_factors(self):
        """U only (the item tables may live elsewhere: row-sharded multi-GPU mode binds a local shard)"""
        tu, _, k = self.shape
        U = np.empty((tu, k), np.float32)
        check(lib().cornac_hip_bpr_get_factors(self.h, U.ctypes.data, None, None))
        return U

    def get_item_factors(self):
        """(V, B) only"""
        _, ti, k = self.shape
        V, B = np.empty((ti, k), np.float32), np.empty(ti, np.float32)
        check(lib().cornac_hip_bpr_get_factors(self.h, None, V.ctypes.data, B.ctypes.data))
        return V, B

    def seed_mt19937(self, seed_pos, seed_neg, shared_stream=False):
        check(lib().cornac_hip_bpr_seed_mt19937(self.h, seed_pos, seed_neg, int(shared_stream)))

    def seed_hogwild(self, seed):
        check(lib().cornac_hip_bpr_seed_hogwild(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def fit_epochs(self, n_epochs, lr, reg, use_bias=True, neg_population=NEG_UNIFORM, mode=MODE_HOGWILD, flags=0):
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_bpr_fit_epochs(self.h, n_epochs, lr, reg, int(use_bias), neg_population, mode, flags,
                                              C.byref(c), C.byref(s)))
        return c.value, s.value

    def hogwild_enqueue(self, n_samples, lr, reg, use_bias=True, neg_population=NEG_UNIFORM, flags=0):
        check(lib().cornac_hip_bpr_hogwild_enqueue(self.h, n_samples, lr, reg, int(use_bias), neg_population, flags))

    def sync(self):
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_bpr_sync(self.h, C.byref(c), C.byref(s)))
        return c.value, s.value

    def bind_device(self, dU=None, dV=None, dB=None):
        check(lib().cornac_hip_bpr_bind_device(self.h, dU, dV, dB))

    def set_negative_population(self, items):
        """population of the popularity-weighted negative draw (WBPR): a multiset of train item ids, e.g. the GLOBAL item
        popularity when this handle holds a user slice; None / empty = the handle's own interactions (recom_wbpr.pyx:135)"""
        items = np.ascontiguousarray(items if items is not None else [], np.int32)
        check(lib().cornac_hip_bpr_set_negative_population(self.h, items.ctypes.data if len(items) else None, len(items)))

    def rebind_items(self, dV, dB):
        """swap the bound (caller-owned) item tables without synchronising the handle's stream"""
        check(lib().cornac_hip_bpr_rebind_items(self.h, dV, dB))

    # ---- conveyor layout (multi-GPU regime 2; cornac_amd/dist.py BinConveyorBprTrainer) ----------------------
    def conveyor_setup(self, n_blocks, rank_item=None, deal_seed=0, release_item_tables=True):
        """-> (n_bins, bins_per_block, cap): see include/cornac_hip.h"""
        order = None if rank_item is None else np.ascontiguousarray(rank_item, np.int32)
        nb, bpb, cap = C.c_int(), C.c_int(), C.c_int()
        check(lib().cornac_hip_bpr_conveyor_setup(self.h, int(n_blocks), None if order is None else order.ctypes.data,
                                                  int(deal_seed) & 0xFFFFFFFFFFFFFFFF, int(bool(release_item_tables)),
                                                  C.byref(nb), C.byref(bpb), C.byref(cap)))
        return nb.value, bpb.value, cap.value

    def conveyor_layout(self, layout_epoch, d_slot_item, d_item_slot):
        check(lib().cornac_hip_bpr_conveyor_layout(self.h, int(layout_epoch), d_slot_item, d_item_slot))

    def conveyor_enqueue(self, epoch, layout_epoch, first_blocks, d_rows, lr, reg, use_bias=True, neg_population=NEG_UNIFORM,
                         flags=0):
        n = len(first_blocks)
        fb = (C.c_int32 * n)(*[int(b) for b in first_blocks])
        rows = (_vp * n)(*[int(p) for p in d_rows])
        check(lib().cornac_hip_bpr_conveyor_enqueue(self.h, int(epoch), int(layout_epoch), n, fb, rows, lr, reg, int(use_bias),
                                                    neg_population, int(flags)))

    def device_ptrs(self):
        u, v, b = _vp(), _vp(), _vp()
        check(lib().cornac_hip_bpr_device_ptrs(self.h, C.byref(u), C.byref(v), C.byref(b)))
        return u.value, v.value, b.value

    def set_stream(self, stream_ptr):
        check(lib().cornac_hip_bpr_set_stream(self.h, stream_ptr))
        self._stream = stream_ptr

    def switch_stream(self, stream_ptr):
        """set_stream without waiting for the previous stream's queued work (the caller orders the streams)"""
        check(lib().cornac_hip_bpr_switch_stream(self.h, stream_ptr))
        self._stream = stream_ptr

    # ---- row-sharded item table building blocks (device pointers; see cornac_amd/dist.py) -----------
    def sample_triplets(self, n_draws, d_u, d_i, d_j, neg_population=NEG_UNIFORM):
        check(lib().cornac_hip_bpr_sample_triplets(self.h, int(n_draws), neg_population, d_u, d_i, d_j))

    def apply_triplets(self, d_u, d_slot_i, d_slot_j, n, d_rows, d_bias, bias_stride, lr, reg, use_bias=True):
        check(lib().cornac_hip_bpr_apply_triplets(self.h, d_u, d_slot_i, d_slot_j, int(n), d_rows, d_bias,
                                                  int(bias_stride), lr, reg, int(use_bias)))

    def staged_slots(self, n_draws):
        """array length emit_triplets needs for n_draws (0: this shape has no owned kernel)"""
        n = C.c_int64()
        check(lib().cornac_hip_bpr_staged_slots(self.h, int(n_draws), C.byref(n)))
        return n.value

    def emit_triplets(self, n_draws, d_u, d_i, d_j, slots_cap, neg_population=NEG_UNIFORM):
        n = C.c_int64()
        check(lib().cornac_hip_bpr_emit_triplets(self.h, int(n_draws), neg_population, d_u, d_i, d_j, int(slots_cap),
                                                 C.byref(n)))
        return n.value

    def apply_staged(self, d_u, d_slot_i, d_slot_j, n_slots, d_rows, d_bias, bias_stride, lr, reg, use_bias=True):
        check(lib().cornac_hip_bpr_apply_staged(self.h, d_u, d_slot_i, d_slot_j, int(n_slots), d_rows, d_bias,
                                                int(bias_stride), lr, reg, int(use_bias)))

    def shard_mark(self, d_i, d_j, n, world, rows_per_rank, d_mark):
        check(lib().cornac_hip_bpr_shard_mark(self.h, d_i, d_j, int(n), int(world), int(rows_per_rank), d_mark))

    def shard_slots(self, d_i, d_j, n, world, rows_per_rank, d_scan, d_slot_i, d_slot_j):
        check(lib().cornac_hip_bpr_shard_slots(self.h, d_i, d_j, int(n), int(world), int(rows_per_rank), d_scan, d_slot_i,
                                               d_slot_j))

    def shard_uniq(self, d_mark, d_scan, n_rows, rows_per_rank, d_uniq_local):
        check(lib().cornac_hip_bpr_shard_uniq(self.h, d_mark, d_scan, int(n_rows), int(rows_per_rank), d_uniq_local))

    def scatter_diff_rows(self, d_table, d_ids, n, width, d_now, d_before, d_scale=None):
        check(lib().cornac_hip_bpr_scatter_diff_rows(self.h, d_table, d_ids, int(n), int(width), d_now, d_before, d_scale))

    # the replicated table's elementwise passes (ItemTableReplica) on the handle's stream (and on its packed records
    # where it keeps them); rule 0 = sqrt through the first entry points, any rule through cornac_hip_bpr_table_delta
    def _delta(self, op, rule, *args):
        check(lib().cornac_hip_bpr_table_delta(self.h, op, int(rule), *args))

    def table_delta_begin(self, d_flat, d_base, n_items, k, d_bucket, d_local, rule=0):
        if rule:
            return self._delta(0, rule, d_flat, d_base, None, None, int(n_items), int(k), d_bucket, d_local)
        check(lib().cornac_hip_bpr_table_delta_begin(self.h, d_flat, d_base, int(n_items), int(k), d_bucket, d_local))

    def table_delta_finish(self, d_flat, d_base, d_bucket, d_local, n_items, k, rule=0):
        if rule:
            return self._delta(1, rule, d_flat, d_base, d_bucket, d_local, int(n_items), int(k), None, None)
        check(lib().cornac_hip_bpr_table_delta_finish(self.h, d_flat, d_base, d_bucket, d_local, int(n_items), int(k)))

    def table_delta_step(self, d_flat, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local, rule=0):
        if rule:
            return self._delta(2, rule, d_flat, d_base, d_bucket_prev, d_local_prev, int(n_items), int(k), d_bucket, d_local)
        check(lib().cornac_hip_bpr_table_delta_step(self.h, d_flat, d_base, d_bucket_prev, d_local_prev, int(n_items),
                                                    int(k), d_bucket, d_local))

    # ---- resident exchange (multi-GPU regime 1 inside one launch per epoch; include/cornac_hip.h) ----
    def resident_exchange_bins(self, neg_population=NEG_UNIFORM, flags=0):
        """workgroups of the resident-exchange launch (= arrivals per exchange); 0: this shape / these flags do not take
        the LDS-bin form and the driver has to cut the epoch into chunk launches"""
        n = C.c_int()
        check(lib().cornac_hip_bpr_resident_exchange_bins(self.h, neg_population, flags, C.byref(n)))
        return n.value

    def epoch_resident_enqueue(self, lr, reg, use_bias, neg_population, flags, n_exchanges, rule, d_base, d_buckets,
                               bucket_stride, d_keeps, keep_stride, d_arrive, d_landed, d_applied):
        n = C.c_int()
        check(lib().cornac_hip_bpr_epoch_resident_enqueue(self.h, lr, reg, int(use_bias), neg_population, flags,
                                                          int(n_exchanges), int(rule), d_base, d_buckets, int(bucket_stride),
                                                          d_keeps, int(keep_stride), d_arrive, d_landed, d_applied, C.byref(n)))
        return n.value

    def resident_flush(self, n_exchanges, rule, d_base, d_buckets, bucket_stride, d_keeps, keep_stride, d_applied, d_landed=None):
        check(lib().cornac_hip_bpr_resident_flush(self.h, int(n_exchanges), int(rule), d_base, d_buckets, int(bucket_stride),
                                                  d_keeps, int(keep_stride), d_applied, d_landed))

    def gather_rows(self, d_table, d_ids, n, width, d_out):
        check(lib().cornac_hip_bpr_gather_rows(self.h, d_table, d_ids, int(n), int(width), d_out))

    def scatter_add_rows(self, d_table, d_ids, n, width, d_delta):
        check(lib().cornac_hip_bpr_scatter_add_rows(self.h, d_table, d_ids, int(n), int(width), d_delta))

    def debug_draw(self, stream, hi, n):
        out = np.empty(n, np.int64)
        check(lib().cornac_hip_bpr_debug_draw(self.h, stream, hi, n, out))
        return out

    def set_views(self, view_indptr, view_indices):
        self.v_indptr = np.ascontiguousarray(view_indptr, np.int32)
        self.v_indices = np.ascontiguousarray(view_indices, np.int32)
        if len(self.v_indices) == 0:
            self.v_indices = np.zeros(1, np.int32)
        check(lib().cornac_hip_bpr_set_views(self.h, self.v_indptr, self.v_indices, int(self.v_indptr[-1])))

    def seed_view_stream(self, seed_view):
        check(lib().cornac_hip_bpr_seed_view_stream(self.h, seed_view))

    def fit_epochs_vebpr(self, n_epochs, lr, reg, alpha, mode=MODE_HOGWILD, ownership=True):
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_vebpr_fit_epochs(self.h, n_epochs, lr, reg, alpha, mode | (0 if ownership else VEBPR_NO_OWNERSHIP),
                                                C.byref(c), C.byref(s)))
        return c.value, s.value

    def fit_epochs_vebpr_f64(self, n_epochs, lr, reg, alpha):
        """float64 tables (set_factors_f64): sequential semantics, everything in double (recom_vebpr.pyx:219)"""
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_vebpr_fit_epochs_f64(self.h, n_epochs, float(lr), float(reg), float(alpha), C.byref(c),
                                                    C.byref(s)))
        return c.value, s.value

    def vebpr_hogwild_owned(self):
        """True if the last VEBPR hogwild epoch ran with user-row ownership (k > 32, enough interactions per wave)"""
        o = C.c_int()
        check(lib().cornac_hip_vebpr_hogwild_form(self.h, C.byref(o)))
        return bool(o.value)

    def mmmf_fit_epochs(self, n_epochs, lr, reg, mode=MODE_HOGWILD):
        """MMMF's hinge loss on this handle (recom_mmmf.pyx:126-158): (correct, skipped) summed over the call"""
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_mmmf_fit_epochs(self.h, n_epochs, lr, reg, mode, C.byref(c), C.byref(s)))
        return c.value, s.value

    def mmmf_fit_epochs_f64(self, n_epochs, lr, reg):
        """float64 tables (set_factors_f64): sequential semantics, everything in double (recom_mmmf.pyx:103-116)"""
        c, s = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_mmmf_fit_epochs_f64(self.h, n_epochs, float(lr), float(reg), C.byref(c), C.byref(s)))
        return c.value, s.value

    def mmmf_hogwild_enqueue(self, n_samples, lr, reg):
        """one MMMF hogwild launch at the current sample offset; sync() collects the counters"""
        check(lib().cornac_hip_mmmf_hogwild_enqueue(self.h, n_samples, lr, reg))

    def debug_ownership(self):
        """(wave_ptr, own_u, own_i) of the hogwild sampler's user-row ownership, or None if unused"""
        w = C.c_int64()
        check(lib().cornac_hip_bpr_debug_ownership(self.h, C.byref(w), None, None, None))
        if w.value == 0:
            return None
        wp = np.empty(w.value + 1, np.int64)
        ou, oi = np.empty(self.nnz, np.int32), np.empty(self.nnz, np.int32)
        check(lib().cornac_hip_bpr_debug_ownership(self.h, C.byref(w), wp.ctypes.data, ou.ctypes.data,
                                                   oi.ctypes.data))
        return wp, ou, oi

    def ldsbin_config(self, hot_x1000=75, min_candidates=48, max_rounds=4):
        check(lib().cornac_hip_bpr_ldsbin_config(self.h, int(hot_x1000), int(min_candidates), int(max_rounds)))

    def ldsbin_deal_config(self, strata_groups=16, hot_cost_x16=32):
        check(lib().cornac_hip_bpr_ldsbin_deal_config(self.h, int(strata_groups), int(hot_cost_x16)))

    def debug_ldsbin_deal(self, seed, epoch):
        """(bin_of_item, cold_mass, hot_off, hot_u, hot_i) of the deal of `epoch` (test hook)."""
        st = self.ldsbin_stats()
        bins, nh = st["bins"], st["hot_interactions"]
        bin_of = np.empty(self.n_items, np.int32)
        cold, off = np.empty(bins, np.uint32), np.empty(bins + 1, np.uint32)
        hu, hi = np.empty(max(nh, 1), np.int32), np.empty(max(nh, 1), np.int32)
        check(lib().cornac_hip_bpr_debug_ldsbin_deal(self.h, int(seed), int(epoch), bin_of.ctypes.data, cold.ctypes.data,
                                                     off.ctypes.data, hu.ctypes.data, hi.ctypes.data))
        return bin_of, cold, off, hu[:nh], hi[:nh]

    def ldsbin_pass_config(self, enable=True, waves=8, lds_kb=64, min_draws_x100=200):
        """the "passing bins" regime of the LDS-bin form (item tables that need more than max_rounds rounds): see
        include/cornac_hip.h"""
        check(lib().cornac_hip_bpr_ldsbin_pass_config(self.h, int(bool(enable)), int(waves), int(lds_kb), int(min_draws_x100)))

    def ldsbin_stats(self):
        o = (C.c_int64 * 8)()
        check(lib().cornac_hip_bpr_ldsbin_stats(self.h, o))
        return {"bins": o[0], "rows_per_bin": o[1], "n_hot": o[2], "hot_interactions": o[3], "bitmap_words": o[4],
                "lds_bytes": o[5], "lock_timeouts": o[6], "block_threads": o[7]}

    def strata_config(self, hot_permille=120, hot_min_mult_x100=200, rehash_period=1):
        check(lib().cornac_hip_bpr_strata_config(self.h, int(hot_permille), int(hot_min_mult_x100), int(rehash_period)))

    def chunk_records(self, enable=True):
        """let hogwild_enqueue keep the strata form's packed item records from call to call (see include/cornac_hip.h:
        the caller touches the bound dense table only through table_delta_* until sync())"""
        check(lib().cornac_hip_bpr_chunk_records(self.h, int(bool(enable))))

    def strata_stats(self):
        o = (C.c_int64 * 4)()
        check(lib().cornac_hip_bpr_strata_stats(self.h, o))
        return {"n_hot": o[0], "misplaced_workgroups": o[1], "bucket_builds": o[2], "waves": o[3]}

    def debug_strata(self, epoch):
        """(sptr, rec_u, rec_i, rank_item, key): the partition buckets the strata form uses in `epoch`"""
        # (a first call without buffers builds the strata grid's ownership tables, so that this works before any launch)
        check(lib().cornac_hip_bpr_debug_strata(self.h, int(epoch), None, None, None, None, None))
        wp = self.debug_ownership()[0]
        W = len(wp) - 1
        sptr = np.empty(8 * W + 1, np.int64)
        ru, ri = np.empty(self.nnz, np.int32), np.empty(self.nnz, np.int32)
        rank_item = np.empty(self.n_items, np.int32)
        key = C.c_uint32()
        check(lib().cornac_hip_bpr_debug_strata(self.h, int(epoch), sptr.ctypes.data, ru.ctypes.data, ri.ctypes.data,
                                                rank_item.ctypes.data, C.byref(key)))
        return sptr, ru, ri, rank_item, key.value

    def kernel_timing(self, enable=True):
        """(total_ms, launches) of the hogwild kernel launches recorded since the last call (HIP events)."""
        ms, n = C.c_double(), C.c_int64()
        check(lib().cornac_hip_bpr_kernel_timing(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_timing(self):
        t = (C.c_double * 4)()
        check(lib().cornac_hip_bpr_last_timing(self.h, t))
        return {"sampler_ms": t[0], "schedule_ms": t[1], "sgd_ms": t[2], "total_ms": t[3]}


class MfTrainer(_HandleOwner):
    _DESTROY = "cornac_hip_mf_destroy"

    def __init__(self, rid, cid, val, n_users, n_items, k, device=0):
        self.rid = np.ascontiguousarray(rid, np.int64)
        self.cid = np.ascontiguousarray(cid, np.int64)
        self.val = np.ascontiguousarray(val, np.float32)
        self.shape = (int(n_users), int(n_items), int(k))
        self.h = _vp()
        check(lib().cornac_hip_mf_create(C.byref(self.h), device, n_users, n_items, k, self.rid, self.cid, self.val,
                                         len(self.val)))
        self.device, self._stream = int(device), None

    def set_factors(self, U=None, V=None, Bu=None, Bi=None):
        U, V, Bu, Bi = _f32c(U), _f32c(V), _f32c(Bu), _f32c(Bi)
        check(lib().cornac_hip_mf_set_factors(self.h, _ptr(U), _ptr(V), _ptr(Bu), _ptr(Bi)))

    def get_factors(self):
        nu, ni, k = self.shape
        U, V = np.empty((nu, k), np.float32), np.empty((ni, k), np.float32)
        Bu, Bi = np.empty(nu, np.float32), np.empty(ni, np.float32)
        check(lib().cornac_hip_mf_get_factors(self.h, U.ctypes.data, V.ctypes.data, Bu.ctypes.data, Bi.ctypes.data))
        return U, V, Bu, Bi

    def fit(self, max_iter, lr, reg, mu, use_bias=True, early_stop=False, mode=MODE_HOGWILD):
        loss = np.zeros(max(max_iter, 1), np.float32)
        n = C.c_int()
        check(lib().cornac_hip_mf_fit(self.h, max_iter, lr, reg, mu, int(use_bias), int(early_stop), mode,
                                      loss.ctypes.data, C.byref(n)))
        return loss[:n.value], n.value

    def det_form(self):
        """(form, own_user) of the last deterministic epoch: 1 dataflow launch / 2 level schedule / 0 none yet; whether the
        dataflow launch's waves owned the user rows (0 unless form is 1)"""
        form, own = C.c_int(), C.c_int()
        check(lib().cornac_hip_mf_det_form(self.h, C.byref(form), C.byref(own)))
        return form.value, own.value

    # ---- multi-GPU driver surface (cornac_amd/dist.py ShardedMfTrainer) ----------------------------------------
    def bind_items(self, d_V, d_Bi):
        """train into caller-owned device buffers for the item side (the replicated [V | Bi] table)"""
        check(lib().cornac_hip_mf_bind_items(self.h, d_V, d_Bi))

    def bind_users(self, d_U, d_Bu):
        """train into caller-owned device buffers for the user side (dist.MfBlockRotationTrainer: the handles of a rank's item
        blocks share it)"""
        check(lib().cornac_hip_mf_bind_users(self.h, d_U, d_Bu))

    def set_stream(self, hip_stream):
        check(lib().cornac_hip_mf_set_stream(self.h, hip_stream))
        self._stream = hip_stream

    def epoch_enqueue(self, part, n_parts, lr, reg, mu, use_bias=True):
        """ratings [nnz*part/n_parts, nnz*(part+1)/n_parts) of the stored order, no host synchronisation"""
        check(lib().cornac_hip_mf_epoch_enqueue(self.h, int(part), int(n_parts), lr, reg, mu, int(use_bias)))

    def sync(self):
        """wait for the enqueued slices; the sum of squared errors they saw"""
        l = C.c_double()
        check(lib().cornac_hip_mf_sync(self.h, C.byref(l)))
        return l.value

    # the replicated table's elementwise passes (ItemTableReplica), on the stream of set_stream; rule: dist.RULES
    def table_delta_begin(self, d_flat, d_base, n_items, k, d_bucket, d_local, rule=0):
        check(lib().cornac_hip_table_delta(0 | (int(rule) << 4), self.device, self._stream, d_flat, d_base, None, None,
                                           int(n_items), int(k), d_bucket, d_local))

    def table_delta_finish(self, d_flat, d_base, d_bucket, d_local, n_items, k, rule=0):
        check(lib().cornac_hip_table_delta(1 | (int(rule) << 4), self.device, self._stream, d_flat, d_base, d_bucket, d_local,
                                           int(n_items), int(k), None, None))

    def table_delta_step(self, d_flat, d_base, d_bucket_prev, d_local_prev, n_items, k, d_bucket, d_local, rule=0):
        check(lib().cornac_hip_table_delta(2 | (int(rule) << 4), self.device, self._stream, d_flat, d_base, d_bucket_prev,
                                           d_local_prev, int(n_items), int(k), d_bucket, d_local))

    OPTIMIZERS = {"sgd": 0, "adam": 1, "rmsprop": 2, "adagrad": 3}

    def fit_minibatch(self, order, batch_size, optimizer, lr, reg, mu, use_bias=True, keep_u=None, keep_i=None,
                      keep_scale=1.0):
        """one optimiser step per consecutive slice of `batch_size` entries of `order` (indices into the
        rating arrays); returns the summed squared error over all visited ratings.  keep_u / keep_i: the dropout keep
        masks of the gathered user / item rows, uint8 [len(order), k] (row b belongs to order[b]; kept factors are scaled
        by keep_scale); None = no dropout"""
        order = np.ascontiguousarray(order, np.int64)
        loss = C.c_double()
        if keep_u is not None:
            keep_u, keep_i = np.ascontiguousarray(keep_u, np.uint8), np.ascontiguousarray(keep_i, np.uint8)
            if keep_u.shape != (len(order), self.shape[2]) or keep_i.shape != keep_u.shape:
                raise ValueError("keep masks must be [len(order), k] = %r, got %r / %r"
                                 % ((len(order), self.shape[2]), keep_u.shape, keep_i.shape))
            check(lib().cornac_hip_mf_fit_minibatch_dropout(self.h, order, len(order), int(batch_size),
                                                            self.OPTIMIZERS[optimizer], lr, reg, mu, int(use_bias),
                                                            keep_u.ctypes.data, keep_i.ctypes.data, float(keep_scale),
                                                            C.byref(loss)))
            return loss.value
        check(lib().cornac_hip_mf_fit_minibatch(self.h, order, len(order), int(batch_size), self.OPTIMIZERS[optimizer],
                                                lr, reg, mu, int(use_bias), C.byref(loss)))
        return loss.value

    def reset_optimizer(self):
        check(lib().cornac_hip_mf_reset_optimizer(self.h))

    # ---- PMF on the same handle (float64 tables and RMSProp caches beside the float32 MF state) ------------------
    PMF_VARIANTS = {"linear": 0, "non_linear": 1}

    def pmf_set_factors(self, U, V):
        """float64 U [n_users, k], V [n_items, k]; zeroes the RMSProp caches"""
        nu, ni, k = self.shape
        U, V = np.ascontiguousarray(U, np.float64), np.ascontiguousarray(V, np.float64)
        if U.shape != (nu, k) or V.shape != (ni, k):
            raise ValueError("PMF tables must be %r and %r, got %r and %r" % ((nu, k), (ni, k), U.shape, V.shape))
        check(lib().cornac_hip_mf_pmf_set_factors(self.h, U.ctypes.data, V.ctypes.data))

    def pmf_get_factors(self):
        nu, ni, k = self.shape
        U, V = np.empty((nu, k), np.float64), np.empty((ni, k), np.float64)
        check(lib().cornac_hip_mf_pmf_get_factors(self.h, U.ctypes.data, V.ctypes.data))
        return U, V

    def pmf_fit(self, n_epochs, lr, reg, gamma, variant):
        """n_epochs sequential epochs (variant: "linear" / "non_linear" or the ABI's code); the loss of each"""
        loss = np.zeros(max(int(n_epochs), 1), np.float64)
        check(lib().cornac_hip_mf_pmf_fit(self.h, int(n_epochs), lr, reg, gamma, self.PMF_VARIANTS.get(variant, variant),
                                          loss.ctypes.data))
        return loss[:max(int(n_epochs), 0)]

    def pmf_form(self):
        """(form, group) of the last PMF epoch: 1 dataflow launch / 2 level schedule / 0 none yet, ratings per wave pass"""
        form, group = C.c_int(), C.c_int()
        check(lib().cornac_hip_mf_pmf_form(self.h, C.byref(form), C.byref(group)))
        return form.value, group.value

    # ---- NMF on the same handle (float32 tables of its own; the ratings must be stored by user) ---------------------
    def nmf_set_factors(self, U, V, Bu=None, Bi=None):
        """float32 U [n_users, k], V [n_items, k]; Bu / Bi: None = zeros"""
        nu, ni, k = self.shape
        U, V, Bu, Bi = _f32c(U), _f32c(V), _f32c(Bu), _f32c(Bi)
        if U.shape != (nu, k) or V.shape != (ni, k):
            raise ValueError("NMF tables must be %r and %r, got %r and %r" % ((nu, k), (ni, k), U.shape, V.shape))
        if (Bu is not None and Bu.shape != (nu,)) or (Bi is not None and Bi.shape != (ni,)):
            raise ValueError("NMF biases must be (%d,) and (%d,)" % (nu, ni))
        check(lib().cornac_hip_mf_nmf_set_factors(self.h, _ptr(U), _ptr(V), _ptr(Bu), _ptr(Bi)))

    def nmf_get_factors(self):
        nu, ni, k = self.shape
        U, V = np.empty((nu, k), np.float32), np.empty((ni, k), np.float32)
        Bu, Bi = np.empty(nu, np.float32), np.empty(ni, np.float32)
        check(lib().cornac_hip_mf_nmf_get_factors(self.h, U.ctypes.data, V.ctypes.data, Bu.ctypes.data, Bi.ctypes.data))
        return U, V, Bu, Bi

    def nmf_fit(self, n_epochs, lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu, use_bias=False, mode=MODE_HOGWILD):
        """n_epochs multiplicative-update epochs; the loss of each (float64)"""
        loss = np.zeros(max(int(n_epochs), 1), np.float64)
        check(lib().cornac_hip_mf_nmf_fit(self.h, int(n_epochs), lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu,
                                          int(bool(use_bias)), int(mode), loss.ctypes.data))
        return loss[:max(int(n_epochs), 0)]

    def nmf_form(self):
        """(sum_form, bias_form, rows_split) of the last NMF epoch: 1 ordered / 2 free-order sums; 0 no bias pass /
        1 dataflow launch / 2 level schedule; rows summed in more than one piece"""
        o = [C.c_int(), C.c_int(), C.c_int()]
        check(lib().cornac_hip_mf_nmf_form(self.h, *[C.byref(x) for x in o]))
        return tuple(x.value for x in o)

    # ---- HPF on the same handle (float64 shape / rate tables of its own; the ratings must be stored by user) ----------
    HPF_MAX_K = 256

    def hpf_set_tables(self, G_s, G_r, L_s, L_r):
        """float64 G_s, G_r [n_users, k], L_s, L_r [n_items, k]: strictly positive and finite, k <= 256"""
        nu, ni, k = self.shape
        if k > self.HPF_MAX_K:
            raise ValueError("HPF keeps a row's sums in registers: k = %d is above its limit of %d" % (k, self.HPF_MAX_K))
        tables = [np.ascontiguousarray(a, np.float64) for a in (G_s, G_r, L_s, L_r)]
        for a, name, shape in zip(tables, ("G_s", "G_r", "L_s", "L_r"), ((nu, k), (nu, k), (ni, k), (ni, k))):
            if a.shape != shape:
                raise ValueError("HPF table %s must be %r, got %r" % (name, shape, a.shape))
            if not (np.isfinite(a).all() and (a > 0).all()):
                raise ValueError("HPF table %s must be strictly positive and finite" % name)
        check(lib().cornac_hip_mf_hpf_set_tables(self.h, *[a.ctypes.data for a in tables]))

    def hpf_get_tables(self):
        """(G_s, G_r, L_s, L_r, K_r, T_r)"""
        nu, ni, k = self.shape
        out = [np.empty(s, np.float64) for s in ((nu, k), (nu, k), (ni, k), (ni, k), (nu,), (ni,))]
        check(lib().cornac_hip_mf_hpf_get_tables(self.h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def hpf_fit(self, n_iters, hierarchical=True):
        """n_iters variational iterations from the stored tables; K_r / T_r restart as in the reference's routine"""
        check(lib().cornac_hip_mf_hpf_fit(self.h, int(n_iters), int(bool(hierarchical))))

    def hpf_elog(self):
        """(Lt, Lb) = exp(digamma(shape) - log rate) of the current tables"""
        nu, ni, k = self.shape
        Lt, Lb = np.empty((nu, k), np.float64), np.empty((ni, k), np.float64)
        check(lib().cornac_hip_mf_hpf_elog(self.h, Lt.ctypes.data, Lb.ctypes.data))
        return Lt, Lb

    def hpf_form(self):
        """(group, rows_split) of the last HPF iteration: lanes per row (0: none yet), rows summed in more than one piece"""
        o = [C.c_int(), C.c_int()]
        check(lib().cornac_hip_mf_hpf_form(self.h, *[C.byref(x) for x in o]))
        return tuple(x.value for x in o)

    def kernel_timing(self, enable=True):
        ms, n = C.c_double(), C.c_int64()
        check(lib().cornac_hip_mf_kernel_timing(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def hogwild_form(self, form):
        """0 automatic, 1 fused atomic kernel, 2 block rotation (include/cornac_hip.h)"""
        check(lib().cornac_hip_mf_hogwild_form(self.h, int(form)))

    def hogwild_stats(self):
        o = (C.c_int64 * 4)()
        check(lib().cornac_hip_mf_hogwild_stats(self.h, o))
        return {"form_used": o[0], "tiles": o[1], "rows_per_bin": o[2], "gave_up": bool(o[3])}

    def debug_split(self):
        """(split_item, split_ptr): the item rows that train through copies and the copies of each (ids n_items +
        split_ptr[j] .. n_items + split_ptr[j + 1]); empty / [0] when no row is split or nothing has been launched"""
        ns, nv = C.c_int64(), C.c_int64()
        check(lib().cornac_hip_mf_debug_split(self.h, C.byref(ns), C.byref(nv), None, None))
        items, ptr = np.empty(ns.value, np.int32), np.zeros(ns.value + 1, np.int32)
        if ns.value:
            check(lib().cornac_hip_mf_debug_split(self.h, C.byref(ns), C.byref(nv), items.ctypes.data, ptr.ctypes.data))
        return items, ptr

    def debug_ownership(self):
        """(wave_ptr, own_u, own_i) of the fused kernel's user-row ownership, or None if the last hogwild launch was not
        an owned one"""
        w = C.c_int64()
        check(lib().cornac_hip_mf_debug_ownership(self.h, C.byref(w), None, None, None))
        if w.value == 0:
            return None
        wp = np.empty(w.value + 1, np.int64)
        ou, oi = np.empty(len(self.val), np.int32), np.empty(len(self.val), np.int32)
        check(lib().cornac_hip_mf_debug_ownership(self.h, C.byref(w), wp.ctypes.data, ou.ctypes.data, oi.ctypes.data))
        return wp, ou, oi

    def last_timing(self):
        t = (C.c_double * 4)()
        check(lib().cornac_hip_mf_last_timing(self.h, t))
        return {"schedule_ms": t[1], "sgd_ms": t[2], "total_ms": t[3]}


def mf_fit_sgd(rid, cid, val, U, V, Bu, Bi, lr, reg, mu, max_iter, use_bias, early_stop, mode, device=0):
    """One-shot in-place call with the reference's argument list (backend_cpu.pyx:35-40)."""
    loss = np.zeros(max(max_iter, 1), np.float32)
    n = C.c_int()
    check(lib().cornac_hip_mf_fit_sgd(device, np.ascontiguousarray(rid, np.int64), np.ascontiguousarray(cid, np.int64),
                                      np.ascontiguousarray(val, np.float32), len(val), U, V, Bu, Bi, U.shape[0],
                                      V.shape[0], U.shape[1], lr, reg, mu, max_iter, int(use_bias), int(early_stop),
                                      mode, loss.ctypes.data, C.byref(n)))
    return loss[:n.value]


class Scorer(_HandleOwner):
    _DESTROY = "cornac_hip_scorer_destroy"

    def __init__(self, U, V, item_base=None, user_base=None, device=0):
        U, V = _f32c(U), _f32c(V)
        self.n_users, self.k = U.shape
        self.n_items = V.shape[0]
        self.h = _vp()
        check(lib().cornac_hip_scorer_create(C.byref(self.h), device, self.n_users, self.n_items, self.k))
        self.set(U, V, item_base, user_base)

    def set(self, U, V, item_base=None, user_base=None):
        ib, ub = _f32c(item_base), _f32c(user_base)
        check(lib().cornac_hip_scorer_set(self.h, _f32c(U), _f32c(V), _ptr(ib), _ptr(ub)))

    def score_user(self, user):
        out = np.empty(self.n_items, np.float32)
        check(lib().cornac_hip_score_user(self.h, int(user), out))
        return out

    def set_f64(self, U, V, item_base=None, user_base=None):
        """the float64 tables of a model trained in double (fast_dot's ddot variant, fast_dot.pyx:25-43)"""
        U, V = np.ascontiguousarray(U, np.float64), np.ascontiguousarray(V, np.float64)
        assert U.shape == (self.n_users, self.k) and V.shape == (self.n_items, self.k)
        ib = None if item_base is None else np.ascontiguousarray(item_base, np.float64)
        ub = None if user_base is None else np.ascontiguousarray(user_base, np.float64)
        check(lib().cornac_hip_scorer_set_f64(self.h, U.ctypes.data, V.ctypes.data, _ptr(ib), _ptr(ub)))

    def score_user_f64(self, user):
        out = np.empty(self.n_items, np.float64)
        check(lib().cornac_hip_score_user_f64(self.h, int(user), out.ctypes.data))
        return out

    def score_block(self, users):
        users = np.ascontiguousarray(users, np.int32)
        out = np.empty((len(users), self.n_items), np.float32)
        check(lib().cornac_hip_score_block(self.h, users, len(users), out))
        return out

    def score_pairs(self, users, items, clip=None):
        users = np.ascontiguousarray(users, np.int32)
        items = np.ascontiguousarray(items, np.int32)
        out = np.empty(len(users), np.float32)
        lo, hi = (0.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
        check(lib().cornac_hip_score_pairs(self.h, users, items, len(users), int(clip is not None), lo, hi, out))
        return out

    def rank_topk(self, users, topk, exclude=None):
        """exclude: optional (indptr int64[n+1], indices int32) CSR of items to drop per listed user."""
        users = np.ascontiguousarray(users, np.int32)
        items = np.empty((len(users), topk), np.int32)
        scores = np.empty((len(users), topk), np.float32)
        ip = ix = None
        if exclude is not None:
            ip = np.ascontiguousarray(exclude[0], np.int64)
            ix = np.ascontiguousarray(exclude[1], np.int32)
        check(lib().cornac_hip_rank_topk(self.h, users, len(users), topk, _ptr(ip), _ptr(ix), items, scores))
        return items, scores

    def rank_positions(self, users, targets, exclude=None):
        """targets / exclude: CSR `(indptr int64[n+1], indices int32)` per listed user.  Returns per target
        `(greater, pos, ge, score)`: candidates scored strictly higher, its position in the ranked order, candidates
        scored at least as high (itself included), its score — cornac_hip_rank_positions."""
        users = np.ascontiguousarray(users, np.int32)
        tp = np.ascontiguousarray(targets[0], np.int64)
        tx = np.ascontiguousarray(targets[1], np.int32)
        nt = int(tp[-1])
        greater, pos, ge = (np.empty(nt, np.int32) for _ in range(3))
        scores = np.empty(nt, np.float32)
        ip = ix = None
        if exclude is not None:
            ip = np.ascontiguousarray(exclude[0], np.int64)
            ix = np.ascontiguousarray(exclude[1], np.int32)
        check(lib().cornac_hip_rank_positions(self.h, users, len(users), _ptr(ip), _ptr(ix), _ptr(tp), _ptr(tx), greater,
                                              pos, ge, scores))
        return greater, pos, ge, scores

    def set_exclusions(self, indptr=None, indices=None):
        """Keep per-USER exclusion lists on the device: CSR (indptr int64[n_users + 1], indices int32); None drops them."""
        if indptr is None:
            check(lib().cornac_hip_scorer_set_exclusions(self.h, None, None))
            return
        ip = np.ascontiguousarray(indptr, np.int64)
        ix = np.ascontiguousarray(indices, np.int32)
        assert len(ip) == self.n_users + 1
        check(lib().cornac_hip_scorer_set_exclusions(self.h, ip.ctypes.data, _ptr(ix) if len(ix) else None))

    def rank_topk_resident(self, users, topk, fetch=True, timed=False, pinned=False):
        """top-k with the resident exclusion lists.  users: array of user ids, or (u0, n) for a contiguous range.
        fetch=False leaves the results on the device, fetch="items" copies only the item ids back (what the @k metrics
        read); timed=True also returns the HIP-event milliseconds; pinned=True returns views of page-locked memory owned
        by the scorer (faster device-to-host copy, overwritten by the next pinned call)."""
        if isinstance(users, tuple):
            up, u0, n = None, int(users[0]), int(users[1])
        else:
            ua = np.ascontiguousarray(users, np.int32)
            up, u0, n = ua.ctypes.data, 0, len(ua)
        if fetch and pinned:
            # results land in page-locked memory owned by the scorer: the arrays returned are VIEWS of it, overwritten by
            # the next pinned call and valid until close()
            want_scores = fetch != "items"
            nbytes = n * topk * 4 * (2 if want_scores else 1)
            buf = _vp()
            check(lib().cornac_hip_scorer_host_buffer(self.h, nbytes, C.byref(buf)))
            raw = (C.c_char * nbytes).from_address(buf.value)
            items = np.frombuffer(raw, np.int32, n * topk).reshape(n, topk)
            scores = np.frombuffer(raw, np.float32, n * topk, offset=n * topk * 4).reshape(n, topk) if want_scores else None
        else:
            items = np.empty((n, topk), np.int32) if fetch else None
            scores = np.empty((n, topk), np.float32) if fetch and fetch != "items" else None
        ms = C.c_double()
        check(lib().cornac_hip_rank_topk_resident(self.h, up, u0, n, topk, _ptr(items), _ptr(scores),
                                                  C.cast(C.byref(ms), _vp) if timed else None))
        return (items, scores, ms.value) if timed else (items, scores)

    def rank_topk_device_ms(self, u0, n, topk, repeats=1):
        ms = C.c_double()
        check(lib().cornac_hip_rank_topk_device(self.h, u0, n, topk, repeats, C.byref(ms)))
        return ms.value


class VbprTrainer(_HandleOwner):
    _DESTROY = "cornac_hip_vbpr_destroy"
    NAMES = ("Bi", "Gu", "Gi", "Tu", "E", "Bp")

    def __init__(self, features, n_users, n_items, k, k2, device=0):
        self.F = np.ascontiguousarray(features, np.float32)
        assert self.F.shape[0] == n_items
        self.dims = dict(n_users=int(n_users), n_items=int(n_items), k=int(k), k2=int(k2), n_feat=self.F.shape[1])
        self.h = _vp()
        check(lib().cornac_hip_vbpr_create(C.byref(self.h), device, n_users, n_items, k, k2, self.F.shape[1], self.F))

    def _shapes(self):
        d = self.dims
        return {"Bi": (d["n_items"],), "Gu": (d["n_users"], d["k"]), "Gi": (d["n_items"], d["k"]),
                "Tu": (d["n_users"], d["k2"]), "E": (d["n_feat"], d["k2"]), "Bp": (d["n_feat"],)}

    def set_params(self, **params):
        arrs = []
        for n in self.NAMES:
            a = params.get(n)
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(self._shapes()[n]))
            arrs.append(a)
        check(lib().cornac_hip_vbpr_set_params(self.h, *[_ptr(a) for a in arrs]))

    def get_params(self):
        out = {n: np.empty(s, np.float32) for n, s in self._shapes().items()}
        check(lib().cornac_hip_vbpr_get_params(self.h, *[out[n].ctypes.data for n in self.NAMES]))
        return out

    def fit_batches(self, u, i, j, batch_size, lr, lambda_w, lambda_b, lambda_e):
        u, i, j = (np.ascontiguousarray(x, np.int32) for x in (u, i, j))
        nll = C.c_double()
        check(lib().cornac_hip_vbpr_fit_batches(self.h, u, i, j, len(u), batch_size, lr, lambda_w, lambda_b, lambda_e,
                                                C.byref(nll)))
        return nll.value

    def item_tables(self):
        d = self.dims
        th, vb = np.empty((d["n_items"], d["k2"]), np.float32), np.empty(d["n_items"], np.float32)
        check(lib().cornac_hip_vbpr_item_tables(self.h, th, vb))
        return th, vb


class WmfTrainer(_HandleOwner):
    """Resident WMF trainer: CSC rating matrix, U/V and the Adam state live on the device."""
    _DESTROY = "cornac_hip_wmf_destroy"

    def __init__(self, csc, k, device=0):
        csc = csc.tocsc()
        self.n_users, self.n_items = (int(x) for x in csc.shape)
        self.k = int(k)
        self._indptr = np.ascontiguousarray(csc.indptr, np.int64)
        self._rows = np.ascontiguousarray(csc.indices, np.int32)
        self._vals = np.ascontiguousarray(csc.data, np.float32)
        self.h = _vp()
        check(lib().cornac_hip_wmf_create(C.byref(self.h), device, self.n_users, self.n_items, self.k, self._indptr,
                                          self._rows if len(self._rows) else np.zeros(1, np.int32),
                                          self._vals if len(self._vals) else np.zeros(1, np.float32), len(self._vals)))

    def set_factors(self, U, V):
        U = np.ascontiguousarray(np.asarray(U, np.float32).reshape(self.n_users, self.k))
        V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(self.n_items, self.k))
        check(lib().cornac_hip_wmf_set_factors(self.h, U, V))

    def get_factors(self):
        U, V = np.empty((self.n_users, self.k), np.float32), np.empty((self.n_items, self.k), np.float32)
        check(lib().cornac_hip_wmf_get_factors(self.h, U, V))
        return U, V

    def fit_batches(self, batches, lambda_u, lambda_v, a, b, lr):
        """batches: sequence of item-id arrays (1..128 distinct ids each; a repeated id is rejected, HipError, with the
        state untouched); returns the per-step losses"""
        batches = [np.asarray(x, np.int32).ravel() for x in batches]
        if not batches:
            return np.zeros(0)
        ptr = np.zeros(len(batches) + 1, np.int64)
        np.cumsum([len(x) for x in batches], out=ptr[1:])
        ids = np.ascontiguousarray(np.concatenate(batches), np.int32)
        loss = np.zeros(len(batches), np.float64)
        check(lib().cornac_hip_wmf_fit_batches(self.h, ids, ptr, len(batches), lambda_u, lambda_v, a, b, lr,
                                               loss.ctypes.data))
        return loss

    def kernel_timing(self, enabled=True):
        check(lib().cornac_hip_wmf_kernel_timing(self.h, int(enabled)))

    def last_device_ms(self):
        ms = C.c_double()
        check(lib().cornac_hip_wmf_last_timing(self.h, C.byref(ms)))
        return ms.value


KNN_MAX_K = 64   # CORNAC_HIP_KNN_MAX_K


def _csr_arrays(mat):
    """(indptr int64, indices int32, data float64) of a scipy CSR with sorted indices; the arrays are kept alive by the
    caller for the length of the call"""
    mat = mat.tocsr()
    if not mat.has_sorted_indices:
        mat = mat.sorted_indices()
    return (np.ascontiguousarray(mat.indptr, np.int64), np.ascontiguousarray(mat.indices, np.int32),
            np.ascontiguousarray(mat.data, np.float64))


class KnnSimilarity(_HandleOwner):
    """Owner of a cornac_hip_knn_sim_t handle: `compute_similarity` of cornac/models/knn/similarity.pyx:51-105 over the rows
    of a scipy CSR, as a scipy CSR of float64."""
    _DESTROY = "cornac_hip_knn_sim_destroy"

    def __init__(self, W, device=0):
        self.shape = tuple(int(x) for x in W.shape)
        self._csr = _csr_arrays(W)
        self.h = _vp()
        check(lib().cornac_hip_knn_sim_create(C.byref(self.h), device, self.shape[0], self.shape[1],
                                              *[_ptr(a) for a in self._csr]))

    def run(self, rows_per_pass=0):
        """rows_per_pass: rows whose accumulators are held at once (0: chosen from the free device memory)"""
        import scipy.sparse as sp

        check(lib().cornac_hip_knn_sim_run(self.h, int(rows_per_pass)))
        nnz = C.c_int64()
        check(lib().cornac_hip_knn_sim_nnz(self.h, C.byref(nnz)))
        n = self.shape[0]
        indptr, indices, data = np.empty(n + 1, np.int64), np.empty(nnz.value, np.int32), np.empty(nnz.value, np.float64)
        check(lib().cornac_hip_knn_sim_get(self.h, _ptr(indptr), _ptr(indices), _ptr(data)))
        return sp.csr_matrix((data, indices, indptr.astype(np.int32) if nnz.value < 2 ** 31 else indptr), shape=(n, n))


class KnnScorer(_HandleOwner):
    """Owner of a cornac_hip_knn_scorer_t handle: `compute_score` / `compute_score_single` (similarity.pyx:108-201) for the
    neighbour table N [n_items x n_neighbours] and the query table Q [n_users x n_neighbours], both scipy CSR."""
    _DESTROY = "cornac_hip_knn_scorer_destroy"

    MAX_K = KNN_MAX_K

    def __init__(self, N, Q, user_mode, device=0):
        self.n_items, self.n_neighbours = (int(x) for x in N.shape)
        self.n_users = int(Q.shape[0])
        assert int(Q.shape[1]) == self.n_neighbours, "N and Q must have the same number of columns"
        n, q = _csr_arrays(N), _csr_arrays(Q)
        self.h = _vp()
        check(lib().cornac_hip_knn_scorer_create(C.byref(self.h), device, self.n_items, self.n_neighbours, self.n_users,
                                                 *[_ptr(a) for a in n + q], int(bool(user_mode))))

    def score_users(self, users, k):
        """weighted averages [n, n_items] float64"""
        return _score_by_ids("cornac_hip_knn_scorer_score_users", self.h, np.float64, users, width=self.n_items, extra=(int(k),))

    def score_pairs(self, users, items, k):
        """weighted averages [n] float64 for the pairs (users[p], items[p])"""
        return _score_by_ids("cornac_hip_knn_scorer_score_pairs", self.h, np.float64, users, items, extra=(int(k),))


class EaseModel(_HandleOwner):
    """Owner of a cornac_hip_ease_t handle: X (users x items, scipy CSR) and the dense items x items float64 table that is
    G, then P, then B of cornac/models/ease/recom_ease.py:72-97, and the scores of :123-126 against it."""
    _DESTROY = "cornac_hip_ease_destroy"

    def __init__(self, X, device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        csr = _csr_arrays(X)
        self.h = _vp()
        check(lib().cornac_hip_ease_create(C.byref(self.h), device, self.n_users, self.n_items, *[_ptr(a) for a in csr]))

    def gram(self):
        check(lib().cornac_hip_ease_gram(self.h))

    def invert(self, lamb):
        check(lib().cornac_hip_ease_invert(self.h, float(lamb)))

    def weights(self, posB):
        check(lib().cornac_hip_ease_weights(self.h, int(bool(posB))))

    def fit(self, lamb, posB):
        """gram, invert, weights in one call"""
        check(lib().cornac_hip_ease_fit(self.h, float(lamb), int(bool(posB))))

    def get_table(self):
        out = np.empty((self.n_items, self.n_items), np.float64)
        check(lib().cornac_hip_ease_get_table(self.h, _ptr(out)))
        return out

    def set_table(self, table):
        table = np.ascontiguousarray(table, np.float64)
        assert table.shape == (self.n_items, self.n_items), "the table is items x items"
        check(lib().cornac_hip_ease_set_table(self.h, _ptr(table)))

    def score_users(self, users):
        """X[users, :] . table: [n, n_items] float64"""
        return _score_by_ids("cornac_hip_ease_score_users", self.h, np.float64, users, width=self.n_items)

    def score_pairs(self, users, items):
        """X[users[p], :] . table[:, items[p]]: [n] float64"""
        return _score_by_ids("cornac_hip_ease_score_pairs", self.h, np.float64, users, items)


class _TableModel(_HandleOwner):
    """Owner of a handle whose parameters are named float32 tables: set_params / get_params / get_state / reset_optimizer over
    the library's `_PREFIX` + those names.  __init__ leaves `names` (the reference's state_dict order, which is the order of
    the native pointer list) and `_shapes` (name -> shape)."""
    _PREFIX = None     # "cornac_hip_vaecf_", ...
    _STATEFUL = None   # the names that have optimiser state, in the native order (None: all of `names`)
    _COUNTERS = 1      # the step counters that get_state returns after its two dicts
    _DESTROY = property(lambda self: self._PREFIX + "destroy")

    def _call(self, what, *args):
        check(getattr(lib(), self._PREFIX + what)(getattr(self, self._HANDLE), *args))

    def _empty(self, names=None):
        return {n: np.empty(self._shapes[n], np.float32) for n in (self.names if names is None else names)}

    def _pointers(self, tables, names=None):
        """the native arguments of a dict of tables; a missing name skips"""
        names = self.names if names is None else names
        return ((_vp * len(names))(*[None if tables.get(n) is None else tables[n].ctypes.data for n in names]),)

    def set_params(self, params):
        tables = {n: np.ascontiguousarray(a, np.float32) for n, a in params.items() if a is not None}
        for n, a in tables.items():
            assert a.shape == self._shapes[n], "%s is %r, not %r" % (n, a.shape, self._shapes[n])
        self._call("set_params", *self._pointers(tables))

    def get_params(self):
        out = self._empty()
        self._call("get_params", *self._pointers(out))
        return out

    def get_state(self):
        """(two dicts of the optimiser's state per stateful table, the step counters)"""
        names = self._STATEFUL or self.names
        a, b, t = self._empty(names), self._empty(names), [C.c_int64() for _ in range(self._COUNTERS)]
        self._call("get_state", *self._pointers(a, names), *self._pointers(b, names), *[C.byref(c) for c in t])
        return (a, b) + tuple(int(c.value) for c in t)

    def reset_optimizer(self):
        self._call("reset_optimizer")


class VaecfModel(_TableModel):
    """Owner of a cornac_hip_vaecf_t handle: the binarised training rows, the ten tables of the reference's VAE
    (cornac/models/vaecf/vaecf.py:37-64) with Adam's moments and step counter, the epoch of vaecf.py:127-144 and the scores
    of recom_vaecf.py:193-202.  Tables travel as dicts keyed by the reference's state_dict names, in its shapes.
    get_state() is (m, v, t): Adam's exp_avg and exp_avg_sq per table, and its step counter."""
    _PREFIX = "cornac_hip_vaecf_"
    _HANDLE = "h_"   # (`h` is the hidden size here)
    NAMES = ("encoder.fc0.weight", "encoder.fc0.bias", "enc_mu.weight", "enc_mu.bias", "enc_logvar.weight", "enc_logvar.bias",
             "decoder.fc0.weight", "decoder.fc0.bias", "decoder.fc1.weight", "decoder.fc1.bias")
    ACTS = ("tanh", "sigmoid", "relu", "relu6", "elu")
    LIKELIHOODS = ("mult", "bern", "gaus", "pois")

    @staticmethod
    def shapes(n_items, k, h):
        return dict(zip(VaecfModel.NAMES, ((h, n_items), (h,), (k, h), (k,), (k, h), (k,), (h, k), (h,), (n_items, h), (n_items,))))

    def __init__(self, X, k, h, act_fn="tanh", likelihood="mult", device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.k, self.h = int(k), int(h)
        self.names, self._shapes = self.NAMES, self.shapes(self.n_items, self.k, self.h)
        indptr, indices, _ = _csr_arrays(X)
        self.h_ = _vp()
        check(lib().cornac_hip_vaecf_create(C.byref(self.h_), device, self.n_users, self.n_items, _ptr(indptr), _ptr(indices),
                                            self.k, self.h, self.ACTS.index(act_fn), self.LIKELIHOODS.index(likelihood)))

    def fit_epoch(self, batch_size, lr, beta, eps=None, seed=0):
        """one epoch; eps [n_users, k] is the noise (None: the device generator under `seed`).  Returns (the sum of the
        steps' batch-mean losses, the per-step losses)."""
        if eps is not None:
            eps = np.ascontiguousarray(eps, np.float32)
            assert eps.shape == (self.n_users, self.k)
        steps = np.zeros(max(1, -(-self.n_users // max(int(batch_size), 1))), np.float64)
        total = C.c_double()
        check(lib().cornac_hip_vaecf_fit_epoch(self.h_, int(batch_size), float(lr), float(beta), _ptr(eps),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(total), _ptr(steps)))
        return float(total.value), steps

    def encode_users(self, users):
        """h2 at z = mu: [n, h] float32"""
        return _score_by_ids("cornac_hip_vaecf_encode_users", self.h_, np.float32, users, width=self.h)

    def score_users(self, users):
        """decode(mu(x_u)): [n, n_items] float32"""
        return _score_by_ids("cornac_hip_vaecf_score_users", self.h_, np.float32, users, width=self.n_items)

    def score_pairs(self, users, items):
        return _score_by_ids("cornac_hip_vaecf_score_pairs", self.h_, np.float32, users, items)


class RecvaeModel(_TableModel):
    """Owner of a cornac_hip_recvae_t handle: the training rows with their values, the 53 tables of the reference's VAE
    (cornac/models/recvae/recvae.py:78-84: encoder, prior tables, old encoder, decoder) with the two Adams' moments and step
    counters, the pass of recom_recvae.py:131-145, update_prior (recvae.py:116-117) and the scores of recom_recvae.py:241-278
    in evaluation mode.  Tables travel as dicts keyed by the reference's state_dict names, in its shapes.
    get_state() is (m, v, t_enc, t_dec): Adam's exp_avg and exp_avg_sq per trainable table, and the two step counters."""
    _PREFIX = "cornac_hip_recvae_"
    _HANDLE = "h_"
    _COUNTERS = 2
    ENCODER = tuple("%s%d.%s" % (kind, l, p) for l in range(1, 6) for kind in ("fc", "ln") for p in ("weight", "bias")) + (
        "fc_mu.weight", "fc_mu.bias", "fc_logvar.weight", "fc_logvar.bias")
    PRIORS = ("prior.mu_prior", "prior.logvar_prior", "prior.logvar_uniform_prior")
    NAMES = tuple("encoder." + n for n in ENCODER) + PRIORS + tuple("prior.encoder_old." + n for n in ENCODER) + (
        "decoder.weight", "decoder.bias")
    TRAINABLE = _STATEFUL = tuple("encoder." + n for n in ENCODER) + ("decoder.weight", "decoder.bias")
    MAX_HIDDEN, MAX_LATENT, MAX_BATCH = 1024, 256, 1024

    @staticmethod
    def shapes(n_items, hidden, latent):
        h, k = int(hidden), int(latent)
        enc = [((h, n_items if l == 1 else h), (h,), (h,), (h,)) for l in range(1, 6)]
        enc = tuple(s for layer in enc for s in layer) + ((k, h), (k,), (k, h), (k,))
        return dict(zip(RecvaeModel.NAMES, enc + ((1, k),) * 3 + enc + ((n_items, k), (n_items,))))

    def __init__(self, X, hidden, latent, device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.hidden, self.latent = int(hidden), int(latent)
        self.names, self._shapes = self.NAMES, self.shapes(self.n_items, self.hidden, self.latent)
        indptr, indices, data = _csr_arrays(X)
        self.nnz = len(indices)
        self.h_ = _vp()
        check(lib().cornac_hip_recvae_create(C.byref(self.h_), device, self.n_users, self.n_items, _ptr(indptr), _ptr(indices),
                                             _ptr(data), self.hidden, self.latent))

    def update_prior(self):
        check(lib().cornac_hip_recvae_update_prior(self.h_))

    def prior_posterior(self):
        """the old encoder's cached (mu, logvar) of every user: [n_users, latent] float32 each"""
        mu, lv = (np.empty((self.n_users, self.latent), np.float32) for _ in range(2))
        check(lib().cornac_hip_recvae_get_prior_posterior(self.h_, _ptr(mu), _ptr(lv)))
        return mu, lv

    def fit_epoch(self, order, batch_size, lr, gamma, beta, dropout_rate, step_encoder, step_decoder, keep=None, eps=None, seed=0):
        """one pass over the users in `order`; keep [nnz] uint8 is the dropout mask per stored entry, eps [n_users, latent]
        the noise (None: the device generator under `seed`).  Returns the steps' (mll, kld, negative_elbo): [steps, 3]."""
        order = np.ascontiguousarray(order, np.int32)
        assert order.shape == (self.n_users,)
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8)
            assert keep.shape == (self.nnz,)
        if eps is not None:
            eps = np.ascontiguousarray(eps, np.float32)
            assert eps.shape == (self.n_users, self.latent)
        steps = np.zeros((max(1, -(-self.n_users // max(int(batch_size), 1))), 3), np.float64)
        check(lib().cornac_hip_recvae_fit_epoch(self.h_, _ptr(order), int(batch_size), float(lr), float(gamma or 0.0), float(beta or 0.0),
                                                float(dropout_rate), int(bool(step_encoder)), int(bool(step_decoder)), _ptr(keep),
                                                _ptr(eps), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(steps)))
        return steps

    def encode_users(self, users, with_logvar=False):
        """mu(x_u) without dropout: [n, latent] float32 (and logvar)"""
        users = np.ascontiguousarray(users, np.int32)
        mu = np.empty((len(users), self.latent), np.float32)
        lv = np.empty((len(users), self.latent), np.float32) if with_logvar else None
        check(lib().cornac_hip_recvae_encode_users(self.h_, _ptr(users), len(users), _ptr(mu), _ptr(lv)))
        return (mu, lv) if with_logvar else mu

    def score_users(self, users):
        """decoder(mu(x_u)), the logits: [n, n_items] float32"""
        return _score_by_ids("cornac_hip_recvae_score_users", self.h_, np.float32, users, width=self.n_items)

    def score_pairs(self, users, items):
        return _score_by_ids("cornac_hip_recvae_score_pairs", self.h_, np.float32, users, items)


BIVAE_RANGE = 512   # CORNAC_HIP_BIVAE_RANGE: rows of the other side's table per workgroup of the fused decode's dense pass


class BivaeModel(_TableModel):
    """Owner of a cornac_hip_bivae_t handle: the binarised training matrix in both orientations, the 12 tables of the
    reference's BiVAE (cornac/models/bivaecf/bivae.py:66-86) with Adam's moments and the two step counters, the factor tables
    theta, beta, mu_theta, mu_beta (bivae.py:48-53), the epoch of bivae.py:194-256, the final passes of :258-274 and the
    scores of recom_bivaecf.py:217-224.  Tables travel as dicts keyed by the reference's state_dict names, in its shapes.
    get_state() is (m, v, t_user, t_item): Adam's exp_avg and exp_avg_sq per table, and the two optimisers' step counters."""
    _PREFIX = "cornac_hip_bivae_"
    _HANDLE = "h_"   # (`h` is the hidden size here)
    _COUNTERS = 2
    NAMES = ("user_encoder.fc0.weight", "user_encoder.fc0.bias", "user_mu.weight", "user_mu.bias", "user_std.weight",
             "user_std.bias", "item_encoder.fc0.weight", "item_encoder.fc0.bias", "item_mu.weight", "item_mu.bias",
             "item_std.weight", "item_std.bias")
    FACTORS = ("theta", "beta", "mu_theta", "mu_beta")
    ACTS = ("tanh", "sigmoid", "relu", "relu6", "elu")
    LIKELIHOODS = ("bern", "gaus", "pois")
    RANGE = BIVAE_RANGE

    @staticmethod
    def shapes(n_users, n_items, k, h):
        side = lambda n: ((h, n), (h,), (k, h), (k,), (k, h), (k,))   # noqa: E731
        return dict(zip(BivaeModel.NAMES, side(n_items) + side(n_users)))

    @staticmethod
    def factor_shapes(n_users, n_items, k):
        return dict(zip(BivaeModel.FACTORS, ((n_users, k), (n_items, k), (n_users, k), (n_items, k))))

    def __init__(self, X, k, h, act_fn="tanh", likelihood="pois", device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.k, self.h = int(k), int(h)
        self.names, self._shapes = self.NAMES, self.shapes(self.n_users, self.n_items, self.k, self.h)
        indptr, indices, _ = _csr_arrays(X)
        self.h_ = _vp()
        check(lib().cornac_hip_bivae_create(C.byref(self.h_), device, self.n_users, self.n_items, _ptr(indptr), _ptr(indices),
                                            self.k, self.h, self.ACTS.index(act_fn), self.LIKELIHOODS.index(likelihood)))

    def set_factors(self, theta=None, beta=None, mu_theta=None, mu_beta=None):
        sh = self.factor_shapes(self.n_users, self.n_items, self.k)
        tabs = [_f32c(a) for a in (theta, beta, mu_theta, mu_beta)]
        for n, a in zip(self.FACTORS, tabs):
            assert a is None or a.shape == sh[n], "%s is %r, not %r" % (n, a.shape, sh[n])
        check(lib().cornac_hip_bivae_set_factors(self.h_, *[_ptr(a) for a in tabs]))

    def get_factors(self):
        """{theta, beta, mu_theta, mu_beta}"""
        sh = self.factor_shapes(self.n_users, self.n_items, self.k)
        out = {n: np.empty(sh[n], np.float32) for n in self.FACTORS}
        check(lib().cornac_hip_bivae_get_factors(self.h_, *[_ptr(out[n]) for n in self.FACTORS]))
        return out

    def n_steps(self, batch_size):
        """(item steps, user steps) of an epoch"""
        bs = max(int(batch_size), 1)
        return -(-self.n_items // bs), -(-self.n_users // bs)

    def fit_epoch(self, batch_size, lr, beta_kl, eps_item=None, eps_user=None, seed=0):
        """one epoch: the item steps, then the user steps.  eps_item [2, n_items, k] and eps_user [2, n_users, k] are the noise
        of the training forward (plane 0) and of the forward after the step (plane 1); None: the device generator under
        `seed`.  Returns (the sum of the item steps' batch-mean losses, that of the user steps, the per-step losses, item
        steps first)."""
        eps = []
        for e, n in ((eps_item, self.n_items), (eps_user, self.n_users)):
            if e is not None:
                e = np.ascontiguousarray(e, np.float32)
                assert e.shape == (2, n, self.k)
            eps.append(e)
        steps = np.zeros(sum(self.n_steps(batch_size)), np.float64)
        li, lu = C.c_double(), C.c_double()
        check(lib().cornac_hip_bivae_fit_epoch(self.h_, int(batch_size), float(lr), float(beta_kl), _ptr(eps[0]), _ptr(eps[1]),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(li), C.byref(lu), _ptr(steps)))
        return float(li.value), float(lu.value), steps

    def last_timing(self):
        """(item pass, user pass) of the last fit_epoch in seconds of device time"""
        ti, tu = C.c_double(), C.c_double()
        check(lib().cornac_hip_bivae_last_timing(self.h_, C.byref(ti), C.byref(tu)))
        return ti.value * 1e-3, tu.value * 1e-3

    def infer_means(self):
        check(lib().cornac_hip_bivae_infer_means(self.h_))

    def score_users(self, users):
        """sigmoid(mu_theta[u] . mu_beta^T): [n, n_items] float32"""
        return _score_by_ids("cornac_hip_bivae_score_users", self.h_, np.float32, users, width=self.n_items)

    def score_pairs(self, users, items):
        return _score_by_ids("cornac_hip_bivae_score_pairs", self.h_, np.float32, users, items)


class NcfModel(_TableModel):
    """Owner of a cornac_hip_ncf_t handle: the training CSR with its values, the tables of the reference's GMF / MLP / NeuMF
    module (cornac/models/ncf/backend_pt.py:22-175) with the learner's state and step counter, the epoch of
    recom_ncf_base.py:266-281 over given or device-drawn samples, and the scores of the three _score_pt.  Tables travel as
    dicts keyed by the reference's state_dict names, in its shapes.  get_state() is (s1, s2, t): adam's exp_avg and exp_avg_sq,
    rmsprop's square_avg or adagrad's sum in s1, and the step counter."""
    _PREFIX = "cornac_hip_ncf_"
    KINDS = ("GMF", "MLP", "NeuMF")
    ACTS = ("sigmoid", "tanh", "elu", "selu", "relu", "relu6", "leaky_relu")
    LEARNERS = ("adam", "sgd", "rmsprop", "adagrad")
    MAX_STEP = 16384   # samples of one step: batch_size * (1 + num_neg)

    @staticmethod
    def NAMES(kind, layers=()):
        gmf = ("user_embedding.weight", "item_embedding.weight", "logit.weight", "logit.bias")
        mlp = ("user_embedding.weight", "item_embedding.weight") + tuple(
            "mlp_model.%d.%s" % (2 * l, p) for l in range(max(len(layers) - 1, 0)) for p in ("weight", "bias")) + ("logit.weight", "logit.bias")
        if kind == "GMF":
            return gmf
        if kind == "MLP":
            return mlp
        return ("logit.weight", "logit.bias") + tuple("gmf." + n for n in gmf) + tuple("mlp." + n for n in mlp)

    @staticmethod
    def UNUSED(kind):
        """the tables that forward() does not use: no gradient, no update"""
        return ("gmf.logit.weight", "gmf.logit.bias", "mlp.logit.weight", "mlp.logit.bias") if kind == "NeuMF" else ()

    @staticmethod
    def shapes(kind, n_users, n_items, num_factors=0, layers=()):
        f, layers = int(num_factors), tuple(int(x) for x in layers)
        gmf = ((n_users, f), (n_items, f), (1, f), (1,))
        mlp = ()
        if kind != "GMF":
            mlp = ((n_users, layers[0] // 2), (n_items, layers[0] // 2))
            for l in range(len(layers) - 1):
                mlp += ((layers[l + 1], layers[l]), (layers[l + 1],))
            mlp += ((1, layers[-1]), (1,))
        sh = gmf if kind == "GMF" else mlp if kind == "MLP" else ((1, f + layers[-1]), (1,)) + gmf + mlp
        return dict(zip(NcfModel.NAMES(kind, layers), sh))

    def __init__(self, kind, X, num_factors=8, layers=(64, 32, 16, 8), act_fn="relu", device=0):
        self.kind = kind
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.num_factors = 0 if kind == "MLP" else int(num_factors)
        self.layers = () if kind == "GMF" else tuple(int(x) for x in layers)
        self.names = self.NAMES(kind, self.layers)
        self._shapes = self.shapes(kind, self.n_users, self.n_items, self.num_factors, self.layers)
        indptr, indices, data = _csr_arrays(X)
        self.nnz = int(indptr[-1])
        lay = np.ascontiguousarray(self.layers, np.int32)
        self.h = _vp()
        check(lib().cornac_hip_ncf_create(C.byref(self.h), device, self.KINDS.index(kind), self.n_users, self.n_items, _ptr(indptr),
                                          _ptr(indices), _ptr(data), self.num_factors, _ptr(lay) if len(lay) else None, len(lay),
                                          0 if kind == "GMF" else self.ACTS.index(act_fn)))
        n = C.c_int()
        check(lib().cornac_hip_ncf_n_tables(self.h, C.byref(n)))
        assert n.value == len(self.names)

    def fit_epoch(self, step_ptr, users, items, labels, lr, reg=0.0, learner="adam"):
        """one epoch over the given samples, step s being [step_ptr[s], step_ptr[s + 1]).  Returns (the sum of the steps' mean
        losses, the per-step losses)."""
        step_ptr = np.ascontiguousarray(step_ptr, np.int64)
        users, items = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32)
        labels = np.ascontiguousarray(labels, np.float32)
        assert len(step_ptr) >= 2 and len(users) == len(items) == len(labels) == int(step_ptr[-1])
        steps = np.zeros(len(step_ptr) - 1, np.float64)
        total = C.c_double()
        check(lib().cornac_hip_ncf_fit_epoch(self.h, len(steps), _ptr(step_ptr), _ptr(users), _ptr(items), _ptr(labels), float(lr),
                                             float(reg), self.LEARNERS.index(learner), C.byref(total), _ptr(steps)))
        return float(total.value), steps

    def n_steps(self, batch_size):
        return -(-self.nnz // max(int(batch_size), 1))

    def draw_epoch(self, batch_size, num_neg, seed=0, epoch=0):
        """(step_ptr, users, items, labels) of the device sampler's epoch, without training"""
        total = self.nnz * (1 + max(int(num_neg), 0))
        step_ptr = np.zeros(self.n_steps(batch_size) + 1, np.int64)
        users, items, labels = np.empty(total, np.int32), np.empty(total, np.int32), np.empty(total, np.float32)
        check(lib().cornac_hip_ncf_draw_epoch(self.h, int(batch_size), int(num_neg), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              int(epoch) & 0xFFFFFFFFFFFFFFFF, _ptr(step_ptr), _ptr(users), _ptr(items), _ptr(labels)))
        return step_ptr, users, items, labels

    def fit_epoch_sampled(self, batch_size, num_neg, lr, reg=0.0, learner="adam", seed=0, epoch=0):
        """one epoch over exactly draw_epoch's samples, drawn on the device.  Returns as fit_epoch does."""
        steps = np.zeros(max(self.n_steps(batch_size), 1), np.float64)
        total = C.c_double()
        check(lib().cornac_hip_ncf_fit_epoch_sampled(self.h, int(batch_size), int(num_neg), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                     int(epoch) & 0xFFFFFFFFFFFFFFFF, float(lr), float(reg),
                                                     self.LEARNERS.index(learner), C.byref(total), _ptr(steps)))
        return float(total.value), steps

    def score_users(self, users):
        """forward(u, every item): [n, n_items] float32 probabilities"""
        return _score_by_ids("cornac_hip_ncf_score_users", self.h, np.float32, users, width=self.n_items)

    def score_pairs(self, users, items):
        return _score_by_ids("cornac_hip_ncf_score_pairs", self.h, np.float32, users, items)


class LightGcnModel(_TableModel):
    """Owner of a cornac_hip_lightgcn_t handle: the normalised adjacency of the train matrix's bipartite graph
    (cornac/models/lightgcn/lightgcn.py:13-41), the layer-0 tables `feature_dict.user` / `feature_dict.item` with Adam's state
    and step counter, the epoch of recom_lightgcn.py:157-179 over given triplets, and the final embeddings of model(graph)."""
    _PREFIX = "cornac_hip_lightgcn_"
    PIECE = 512        # edges of one piece of a long row: rows above it are summed in pieces, combined in piece order
    MAX_STEP = 16384   # triplets of one step
    NAMES = ("user", "item")

    def __init__(self, X, emb_size=64, num_layers=3, device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.emb_size, self.num_layers = int(emb_size), int(num_layers)
        self.names, self._shapes = self.NAMES, {"user": (self.n_users, self.emb_size), "item": (self.n_items, self.emb_size)}
        indptr, indices, _ = _csr_arrays(X)
        self.nnz = int(indptr[-1])
        self.h = _vp()
        check(lib().cornac_hip_lightgcn_create(C.byref(self.h), device, self.n_users, self.n_items, _ptr(indptr), _ptr(indices),
                                               self.emb_size, self.num_layers))

    def _pointers(self, tables, names=None):
        """(user, item): the native calls take the two tables as arguments of their own"""
        return tuple(_ptr(tables.get(n)) for n in self.NAMES)

    def set_params(self, user=None, item=None):
        user, item = _f32c(user), _f32c(item)
        assert user is None or user.shape == self._shapes["user"], "user is %r" % (user.shape,)
        assert item is None or item.shape == self._shapes["item"], "item is %r" % (item.shape,)
        self._call("set_params", _ptr(user), _ptr(item))

    def get_params(self):
        out = super().get_params()
        return out["user"], out["item"]

    def get_state(self):
        """(m_user, m_item, v_user, v_item, t): Adam's exp_avg and exp_avg_sq and its step counter"""
        m, v, t = super().get_state()
        return m["user"], m["item"], v["user"], v["item"], t

    def fit_epoch(self, step_ptr, users, pos, neg, lr, lambda_reg):
        """one epoch over the given triplets, step s being [step_ptr[s], step_ptr[s + 1]).  Returns the per-step (losses, bpr,
        reg): bpr + lambda_reg * reg, mean softplus, the halved squared norms over the batch size."""
        step_ptr = np.ascontiguousarray(step_ptr, np.int64)
        users, pos, neg = (np.ascontiguousarray(a, np.int32) for a in (users, pos, neg))
        assert len(step_ptr) >= 2 and len(users) == len(pos) == len(neg) == int(step_ptr[-1])
        losses, bpr, reg = (np.zeros(len(step_ptr) - 1, np.float64) for _ in range(3))
        check(lib().cornac_hip_lightgcn_fit_epoch(self.h, len(losses), _ptr(step_ptr), _ptr(users), _ptr(pos), _ptr(neg), float(lr),
                                                  float(lambda_reg), _ptr(losses), _ptr(bpr), _ptr(reg)))
        return losses, bpr, reg

    def propagate(self):
        """(U, V): the final embeddings, the mean of the layers' tables"""
        out = self._empty()
        self._call("propagate", *self._pointers(out))
        return out["user"], out["item"]


class NgcfModel(_TableModel):
    """Owner of a cornac_hip_ngcf_t handle: the graph of cornac/models/ngcf/ngcf.py:14-37 with its edge norms, the tables
    `feature_dict.user` / `feature_dict.item` and every layer's W1 / W2 with Adam's state and step counter, the train-mode epoch
    of recom_ngcf.py:159-184 over given triplets, and the concatenated embeddings of the eval-mode model(graph).  Parameters
    travel as dicts under the reference's state_dict names, in its order (`names`).  get_state() is (m, v, t): Adam's exp_avg
    and exp_avg_sq as dicts like get_params', and its step counter."""
    _PREFIX = "cornac_hip_ngcf_"
    PIECE = 512          # edges of one piece of a long row (the hop is LightGCN's)
    MAX_STEP = 16384     # triplets of one step
    WGRAD_ROWS = 2048    # rows of one chunk of the weight and bias gradients; the chunks' partials are added in chunk order

    @staticmethod
    def param_shapes(n_users, n_items, emb_size, layer_sizes):
        """name -> shape, in the reference's state_dict order: the layers' Linears, then feature_dict.item, feature_dict.user"""
        from collections import OrderedDict

        out, din = OrderedDict(), int(emb_size)
        for l, dout in enumerate(int(x) for x in layer_sizes):
            for w in ("W1", "W2"):
                out["layers.%d.%s.weight" % (l, w)] = (dout, din)
                out["layers.%d.%s.bias" % (l, w)] = (dout,)
            din = dout
        out["feature_dict.item"] = (int(n_items), int(emb_size))
        out["feature_dict.user"] = (int(n_users), int(emb_size))
        return out

    def __init__(self, X, emb_size=64, layer_sizes=(64, 64, 64), dropout_rates=(0.1, 0.1, 0.1), dropout_key=0, device=0):
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.emb_size = int(emb_size)
        self.layer_sizes, self.dropout_rates = [int(x) for x in layer_sizes], [float(x) for x in dropout_rates]
        assert len(self.layer_sizes) == len(self.dropout_rates), "'layer_sizes' and 'dropout_rates' must be of the same size"
        self.dropout_key = int(dropout_key) & 0xFFFFFFFFFFFFFFFF
        self.D = self.emb_size + sum(self.layer_sizes)
        self.shapes = self._shapes = self.param_shapes(self.n_users, self.n_items, self.emb_size, self.layer_sizes)
        self.names = list(self.shapes)
        indptr, indices, _ = _csr_arrays(X)
        self.nnz = int(indptr[-1])
        sizes, rates = np.asarray(self.layer_sizes, np.int32), np.asarray(self.dropout_rates, np.float32)
        self.h = _vp()
        check(lib().cornac_hip_ngcf_create(C.byref(self.h), device, self.n_users, self.n_items, _ptr(indptr), _ptr(indices),
                                           self.emb_size, len(sizes), _ptr(sizes), _ptr(rates), self.dropout_key))

    def _empty(self, names=None):
        from collections import OrderedDict

        return OrderedDict(super()._empty(names))

    def _pointers(self, tables, names=None):
        """(user, item, layers[4 L]): the native calls take the two embedding tables as arguments of their own"""
        at = lambda n: None if tables.get(n) is None else tables[n].ctypes.data   # noqa: E731
        layers = (_vp * (4 * len(self.layer_sizes)))(*[at("layers.%d.%s" % (l, s)) for l in range(len(self.layer_sizes))
                                                       for s in ("W1.weight", "W1.bias", "W2.weight", "W2.bias")])
        return at("feature_dict.user"), at("feature_dict.item"), layers

    def fit_epoch(self, step_ptr, users, pos, neg, lr, lambda_reg):
        """one train-mode epoch over the given triplets, step s being [step_ptr[s], step_ptr[s + 1]).  Returns the per-step
        (losses, bpr, reg) as LightGcnModel.fit_epoch does."""
        step_ptr = np.ascontiguousarray(step_ptr, np.int64)
        users, pos, neg = (np.ascontiguousarray(a, np.int32) for a in (users, pos, neg))
        assert len(step_ptr) >= 2 and len(users) == len(pos) == len(neg) == int(step_ptr[-1])
        losses, bpr, reg = (np.zeros(len(step_ptr) - 1, np.float64) for _ in range(3))
        check(lib().cornac_hip_ngcf_fit_epoch(self.h, len(losses), _ptr(step_ptr), _ptr(users), _ptr(pos), _ptr(neg), float(lr),
                                              float(lambda_reg), _ptr(losses), _ptr(bpr), _ptr(reg)))
        return losses, bpr, reg

    def propagate(self):
        """(U [n_users x D], V [n_items x D]): the concatenated embeddings in eval mode (no dropout)"""
        user, item = np.empty((self.n_users, self.D), np.float32), np.empty((self.n_items, self.D), np.float32)
        check(lib().cornac_hip_ngcf_propagate(self.h, _ptr(user), _ptr(item)))
        return user, item

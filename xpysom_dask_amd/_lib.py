"""ctypes binding of libsomhip.so (include/somhip.h).  There is no fallback:
if the HIP library is missing or does not load, importing the engine fails."""
import ctypes as C
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOM_LIB_PATH") or os.path.join(HERE, "libsomhip.so")   # override: kernel A/B builds

SOM_DIST = {"euclidean": 0, "euclidean_no_opt": 1, "cosine": 2, "manhattan": 3, "manhattan_no_opt": 3,
            "norm_p": 4, "norm_p_no_opt": 5}
SOM_NEIGH = {"gaussian": 0, "mexican_hat": 1, "bubble": 2, "triangle": 3}
SOM_PREC = {"f32": 0, "bf16": 1, "f16": 3, "exact": 5}      # (ids 2 and 4: the retired split-operand modes)
SOM_TOPO = {"rectangular": 0, "hexagonal": 1, "toroidal": 2}
SOM_MISSING = {None: 0, "nan": 1}
SOM_BMU_ACTIVATION, SOM_BMU_QUANTIZATION = 0, 1
SOM_KERNELS = {"bmu": 0, "segsum": 1, "kron": 2, "merge": 3, "prep": 4, "screen": 5, "fill": 6}


class SomConfig(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("input_len", C.c_int32),
                ("distance", C.c_int32), ("neighborhood", C.c_int32),
                ("compact_support", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32),
                ("std_coeff", C.c_double), ("stream", C.c_void_p),
                ("topology", C.c_int32), ("norm_p", C.c_int32), ("norm_p_real", C.c_double),
                ("missing", C.c_int32)]


class EpochMetrics(C.Structure):
    """som_epoch_metrics_t (include/somhip.h): the training monitor's record of one epoch as the device holds it."""
    _fields_ = [("sum_wd", C.c_double), ("sum_w", C.c_double), ("shift_sumsq", C.c_double),
                ("rows", C.c_int64), ("changed", C.c_int64), ("shift_max", C.c_float)]


_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_H = C.c_void_p

# name -> (restype, argtypes); exactly the symbols include/somhip.h declares
SIGNATURES = {
    "som_version": (C.c_char_p, []),
    "som_device_count": (C.c_int, []),
    "som_last_error": (C.c_char_p, [_H]),
    "som_create": (C.c_int, [C.POINTER(SomConfig), C.POINTER(_H)]),
    "som_destroy": (None, [_H]),
    "som_set_weights": (C.c_int, [_H, _F]),
    "som_get_weights": (C.c_int, [_H, _F]),
    "som_set_data": (C.c_int, [_H, _F, C.c_int64]),
    "som_set_data_device": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "som_set_sample_weights": (C.c_int, [_H, _F, C.c_int64]),
    "som_set_sample_weights_device": (C.c_int, [_H, C.c_void_p, C.c_int64]),
    "som_sync_producer": (C.c_int, [_H, C.c_uint64, C.c_int32]),
    "som_copy_to_host": (C.c_int, [_H, C.c_void_p, C.c_uint64, C.c_void_p]),
    "som_epoch_accumulate": (C.c_int, [_H, C.c_double, C.c_double, C.c_int]),
    "som_epoch_accumulate_faithful": (C.c_int, [_H, C.c_double, C.c_double, C.c_int]),
    "som_epoch_merge": (C.c_int, [_H]),
    "som_epoch": (C.c_int, [_H, C.c_double, C.c_double, C.c_int]),
    "som_epoch_accumulate_begin": (C.c_int, [_H, C.c_double, C.c_double, C.c_int]),
    "som_epoch_block_count": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "som_epoch_accumulate_block": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_comm_load": (C.c_int, [C.c_char_p]),
    "som_comm_unique_id": (C.c_int, [C.c_void_p]),
    "som_comm_init": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p]),
    "som_epoch_allreduce": (C.c_int, [_H]),
    "som_comm_destroy": (C.c_int, [_H]),
    "som_pinned_alloc": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "som_pinned_free": (C.c_int, [C.c_void_p]),
    "som_stream_begin": (C.c_int, [_H]),
    "som_stream_rows": (C.c_int, [_H, _F, C.c_int64]),
    "som_stream_rows_weighted": (C.c_int, [_H, _F, _F, C.c_int64]),
    "som_stream_end": (C.c_int, [_H, C.c_double, C.c_double, C.c_int]),
    "som_accum_device_ptr": (C.c_int, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "som_get_stream": (C.c_int, [_H, C.POINTER(C.c_void_p)]),
    "som_epoch_fetch": (C.c_int, [_H, _F, _F, _I]),
    "som_epoch_fetch_masked": (C.c_int, [_H, _F, _F, _I]),
    "som_epoch_accumulate_forced": (C.c_int, [_H, _I, C.c_double, C.c_double, C.c_int]),
    "som_bmu": (C.c_int, [_H, _F, C.c_int64, C.c_int32, _I]),
    "som_bmu_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, _I]),
    "som_bmu_top2": (C.c_int, [_H, _F, C.c_int64, _I, _I]),
    "som_bmu_top2_device": (C.c_int, [_H, C.c_void_p, C.c_int64, _I, _I]),
    "som_bmu_f64": (C.c_int, [_H, C.POINTER(C.c_double), C.c_int64, _I]),
    "som_distance_matrix": (C.c_int, [_H, _F, C.c_int64, C.c_int32, _F]),
    "som_quantization_error": (C.c_int, [_H, _F, C.c_int64, C.POINTER(C.c_double)]),
    "som_quantization_error_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]),
    "som_bmu_distances": (C.c_int, [_H, _F, C.c_int64, _I, _F]),
    "som_bmu_distances_device": (C.c_int, [_H, C.c_void_p, C.c_int64, _I, _F]),
    "som_unit_stats": (C.c_int, [_H, _F, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), _F]),
    "som_unit_stats_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), _F]),
    "som_impute": (C.c_int, [_H, _F, C.c_int64, _F, _I]),
    "som_impute_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, _I]),
    "som_unit_label_counts": (C.c_int, [_H, _F, _I, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_unit_label_counts_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_unit_value_sums": (C.c_int, [_H, _F, _F, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "som_unit_value_sums_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double)]),
    "som_unit_density": (C.c_int, [_H, _F, C.c_int64, _F, _F, C.c_int32, C.POINTER(C.c_int64)]),
    "som_unit_density_device": (C.c_int, [_H, C.c_void_p, C.c_int64, _F, _F, C.c_int32, C.POINTER(C.c_int64)]),
    "som_debug_density_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_bmu_topk": (C.c_int, [_H, _F, C.c_int64, C.c_int32, C.POINTER(C.c_int32), _F, _F]),
    "som_bmu_topk_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32), _F, _F]),
    "som_unit_rank_counts": (C.c_int, [_H, _F, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_unit_rank_counts_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_debug_topk_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_row_moments": (C.c_int, [_H, _F, _F, C.c_int64, _F, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "som_row_moments_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, _F, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "som_gather_rows_device": (C.c_int, [_H, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int64, _F]),
    "som_debug_moments_plan": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "som_monitor": (C.c_int, [_H, C.c_int32]),
    "som_epoch_measure_rows": (C.c_int, [_H]),
    "som_epoch_measure_shift": (C.c_int, [_H]),
    "som_epoch_metrics": (C.c_int, [_H, C.POINTER(EpochMetrics)]),
    "som_set_verify": (C.c_int, [_H, C.c_int32]),
    "som_verify_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_corrupt_operands": (C.c_int, [_H, C.c_int32]),
    "som_debug_operand_crc": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64)]),
    "som_debug_exact_centroids": (C.c_int, [_H, C.c_int32, _F, _F, _F, _I]),
    "som_debug_mfma16": (C.c_int, [_H, C.c_void_p, C.c_void_p, _F, _F, C.c_int32]),
    "som_debug_radix_sort": (C.c_int, [_H, _I, C.c_int64, C.c_int32, _I, _I]),
    "som_debug_exact_select2": (C.c_int, [_H, _I, C.POINTER(C.c_uint32), C.c_int64, _I, C.POINTER(C.c_uint32), C.c_int32, C.c_int64, _I]),
    "som_debug_exact_tiles": (C.c_int, [_H, _I, _I, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int64, _I, _I, _I]),
    "som_debug_stamps": (C.c_int, [_H, C.c_int64, C.c_void_p]),
    "som_debug_device_bytes": (C.c_int, [C.POINTER(C.c_int64)]),
    "som_debug_qe_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_exact_chain_stats": (C.c_int, [_H, C.POINTER(C.c_int64)]),
    "som_debug_exact_select_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_exact_plan_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_exact_plan_fold_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_plan_split": (C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "som_debug_band_tables": (C.c_int, [_H, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "som_debug_band_walk": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _I, _I]),
    "som_debug_band_tables_wrap": (C.c_int, [_H, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "som_debug_band_walk_wrap": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _I, _I]),
    "som_debug_exact_last_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "som_debug_exact_forecast": (C.c_int, [_H, C.POINTER(C.c_double)]),
    "som_debug_exact_tile_blocks": (C.c_int, [_H, _I, _I, C.c_int64, _I]),
    "som_policy_eval": (C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "som_policy_replay": (C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "som_operands_replay": (C.c_int, [_I, C.c_int32, _I, _I]),
    "som_debug_row_set_sizes": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "som_debug_unit_sort_sizes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "som_debug_unit_sort_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_debug_exact_scratch_sizes": (C.c_int, [C.POINTER(C.c_int64), C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "som_debug_exact_scratch_held": (C.c_int, [_H, C.POINTER(C.c_int64)]),
    "som_patch_order": (C.c_int, [C.c_int32, C.c_int32, _I]),
    "som_exact_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_top2_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_skip_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_resident_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_scout_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_refine_stats": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "som_exact_last_counts": (C.c_int, [_H, _I, C.c_int64]),
    "som_sync": (C.c_int, [_H]),
    "som_profile_enable": (C.c_int, [_H, C.c_int32]),
    "som_profile_get": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "som_profile_reset": (C.c_int, [_H]),
}

_lib = None


def torch_lib_file(name):
    """Path of a library bundled with torch (or None): the copy this process must share with torch."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
    return cand if os.path.exists(cand) else None


def _preload_torch_hip_runtime():
    """torch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).
    If torch is (or will be) imported in this process -- it is, for multi-GPU runs --
    both libraries must resolve to ONE HIP runtime, or streams/pointers handed across
    would belong to different runtimes.  Loading torch's copy first makes the loader
    satisfy libsomhip's DT_NEEDED libamdhip64.so.7 with it."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m xpysom_dask_amd.build` "
            "(needs hipcc; there is no CPU fallback)")
    if not os.environ.get("SOM_LIB_PATH"):             # (an explicit A/B build is the caller's business)
        from . import build as _build
        have, want = _build.built_hash(LIB_PATH), _build.source_hash()
        if have != want:
            raise ImportError(
                f"{LIB_PATH} is stale: built from sources {have}, the tree is {want}; "
                "rebuild with `python -m xpysom_dask_amd.build`")
    _preload_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib

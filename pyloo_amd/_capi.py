"""ctypes binding of libpyloo_amd.so (include/pyloo_amd.h) -- the only way the Python front
reaches the GPU.  There is deliberately no CPU fallback: a missing library or GPU raises."""

import ctypes as C
import os

import numpy as np

PLA_F64, PLA_F32 = 0, 1
PLA_HOST, PLA_DEVICE = 0, 1
PLA_PSIS, PLA_SIS, PLA_TIS = 0, 1, 2
METHOD_CODES = {"psis": PLA_PSIS, "sis": PLA_SIS, "tis": PLA_TIS}
AGG_N, AGG_SUM_LOO, AGG_M2_LOO, AGG_SUM_LPPD, AGG_N_HIGH, AGG_N_NONFINITE, AGG_MIN_DIAG, AGG_N_SLOW = range(8)
AGG_COUNT = 8
ABI_VERSION = 7
PLA_MVN_NORMAL, PLA_MVN_STUDENT_T = 0, 1
PLA_PIT_LOGLIK, PLA_PIT_LOG_WEIGHTS = 0, 1  # input_kind of pla_loo_pit
PLA_ESS_LOG, PLA_ESS_SPLIT, PLA_ESS_CAP = 1, 2, 4  # flags of pla_relative_eff
PLA_LFO_BACKWARD = 0x100  # OR-ed into the method of pla_lfo: backward mode, `first` carries `last`
PLA_NONFACTOR_MAX_OBS = 1024
# status word of a draw of pla_nonfactor_loglik
NF_GENERAL, NF_SINGULAR, NF_NONFINITE, NF_DF_NONPOS, NF_BETA_NONFINITE, NF_CLAMPED = 1, 2, 4, 8, 16, 32
PLA_MM_MAX_COV_DIM, PLA_MM_MAX_DIM = 64, 1024  # pla_mm_moments / pla_mm_transform: D with and without matrices
NF_ROUTE_AUTO, NF_ROUTE_LDS, NF_ROUTE_WORKSPACE, NF_ROUTE_GENERAL = 0, 1, 2, 3

# every symbol declared in include/pyloo_amd.h
SYMBOLS = (
    "pla_abi_version", "pla_last_error", "pla_device_count", "pla_engine_create", "pla_engine_destroy",
    "pla_tail_count", "pla_psis_loo", "pla_importance_weights", "pla_reduce_pointwise", "pla_waic",
    "pla_psis_loo_rows", "pla_waic_rows", "pla_e_loo", "pla_e_loo_quantiles",
    "pla_engine_set_frozen", "pla_engine_set_timing", "pla_engine_kernel_ms", "pla_engine_first_kernel_ms", "pla_fill_synthetic",
    "pla_engine_last_kernels", "pla_aggregate_pack", "pla_aggregate_merge", "pla_fill_synthetic_chains",
    "pla_env_overrides", "pla_engine_stream_stats", "pla_group_sum", "pla_psis_loo_groups",
    "pla_compare_moments", "pla_stacking_eval", "pla_bb_bootstrap", "pla_bb_gamma_draws", "pla_engine_set_compare_grid",
    "pla_nonfactor_loglik", "pla_engine_set_nonfactor_route", "pla_engine_set_nonfactor_grid", "pla_nonfactor_lds_max_obs",
    "pla_gather_draws", "pla_psis_loo_draws", "pla_gather_lds_max_draws",
    "pla_kfold_lme", "pla_kfold_reduce",
    "pla_mm_moments", "pla_mm_transform", "pla_mm_ratios",
    "pla_mixis_draw_lse", "pla_mixis_loo", "pla_engine_set_mixis_grid", "pla_mixis_tile_rows",
    "pla_loo_pit", "pla_lfo_ratios", "pla_lfo",
    "pla_loo_diag", "pla_loo_diag_weights", "pla_loo_influence", "pla_glm", "pla_glm_grouped",
    "pla_glm_marginal", "pla_glm_marginal_segment", "pla_glm_predict", "pla_glm_predict_segment",
    "pla_relative_eff", "pla_engine_set_ess_grid", "pla_ess_lds_max_draws",
)


class InfluenceArgs(C.Structure):
    """``pla_influence_args`` of include/pyloo_amd.h (``struct_size`` is set on construction)."""

    _fields_ = [
        ("struct_size", C.c_int64), ("engine", C.c_void_p), ("mat", C.c_void_p),
        ("dtype", C.c_int32), ("kind", C.c_int32), ("method", C.c_int32), ("mem_space", C.c_int32),
        ("n_obs", C.c_int64), ("n_draws", C.c_int64), ("stride_obs", C.c_int64), ("stride_draw", C.c_int64),
        ("row_index", C.c_void_p), ("n_rows", C.c_int64), ("tail_count", C.c_int64),
        ("theta", C.c_void_p), ("n_quant", C.c_int64), ("theta_stride_draw", C.c_int64), ("theta_stride_quant", C.c_int64),
        ("center", C.c_void_p), ("scale", C.c_void_p), ("stream", C.c_void_p),
        ("shift", C.c_void_p), ("m2", C.c_void_p), ("kl", C.c_void_p), ("ess_w", C.c_void_p), ("diag", C.c_void_p),
        ("n_replaced", C.c_void_p),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(InfluenceArgs)


PLA_GLM_LINPRED, PLA_GLM_GAUSSIAN, PLA_GLM_BINOMIAL_LOGIT, PLA_GLM_POISSON_LOG = 0, 1, 2, 3
PLA_GLM_NEGBINOMIAL_LOG, PLA_GLM_GAMMA_LOG, PLA_GLM_BINOMIAL_PROBIT = 4, 5, 6
PLA_GLM_MODE_MATRIX, PLA_GLM_MODE_LOO = 0, 1
GLM_MAX_PRED = 256


class GlmArgs(C.Structure):
    """``pla_glm_args`` of include/pyloo_amd.h (``struct_size`` is set on construction)."""

    _fields_ = [
        ("struct_size", C.c_int64), ("engine", C.c_void_p),
        ("family", C.c_int32), ("mode", C.c_int32), ("method", C.c_int32), ("mem_space", C.c_int32),
        ("stream", C.c_void_p),
        ("x", C.c_void_p), ("n_obs", C.c_int64), ("n_pred", C.c_int64), ("x_stride_obs", C.c_int64), ("x_stride_pred", C.c_int64),
        ("beta", C.c_void_p), ("n_draws", C.c_int64), ("beta_stride_draw", C.c_int64), ("beta_stride_pred", C.c_int64),
        ("y", C.c_void_p), ("offset", C.c_void_p), ("trials", C.c_void_p), ("obs_const", C.c_void_p),
        ("draw_scale", C.c_void_p), ("draw_const", C.c_void_p),
        ("row_index", C.c_void_p), ("n_rows", C.c_int64), ("tail_count", C.c_int64),
        ("scale_value", C.c_double), ("good_k", C.c_double),
        ("out", C.c_void_p), ("out_pitch", C.c_int64),
        ("diag", C.c_void_p), ("loo_i", C.c_void_p), ("lppd_i", C.c_void_p), ("agg", C.c_void_p),
        ("n_replaced", C.c_void_p),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(GlmArgs)


GLM_MAX_TERMS = 8


class GlmTerm(C.Structure):
    """``pla_glm_term`` of include/pyloo_amd.h."""

    _fields_ = [
        ("group_index", C.c_void_p), ("z", C.c_void_p), ("u", C.c_void_p),
        ("u_stride_draw", C.c_int64), ("u_stride_group", C.c_int64), ("n_groups", C.c_int64),
    ]


class GlmGroupedArgs(C.Structure):
    """``pla_glm_grouped_args`` of include/pyloo_amd.h: ``glm`` is a ``GlmArgs`` (both ``struct_size`` are set on construction)."""

    _fields_ = [("struct_size", C.c_int64), ("glm", GlmArgs), ("n_terms", C.c_int64), ("terms", GlmTerm * GLM_MAX_TERMS)]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(GlmGroupedArgs)
        self.glm.struct_size = C.sizeof(GlmArgs)


GLM_MARGINAL_MAX_NODES = 32


class GlmMarginalArgs(C.Structure):
    """``pla_glm_marginal_args`` of include/pyloo_amd.h: ``grouped`` is a ``GlmGroupedArgs`` (all three ``struct_size`` are set on
    construction)."""

    _fields_ = [
        ("struct_size", C.c_int64), ("grouped", GlmGroupedArgs), ("n_clusters", C.c_int64), ("n_members", C.c_int64),
        ("cluster_offsets", C.c_void_p), ("members", C.c_void_p), ("z", C.c_void_p), ("tau", C.c_void_p),
        ("n_nodes", C.c_int64), ("nodes", C.c_void_p), ("log_weights", C.c_void_p),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(GlmMarginalArgs)
        self.grouped.struct_size = C.sizeof(GlmGroupedArgs)
        self.grouped.glm.struct_size = C.sizeof(GlmArgs)


class GlmPredictArgs(C.Structure):
    """``pla_glm_predict_args`` of include/pyloo_amd.h: ``glm`` is a ``GlmArgs`` (both ``struct_size`` are set on construction)."""

    _fields_ = [
        ("struct_size", C.c_int64), ("glm", GlmArgs), ("kind", C.c_int64), ("log_weights", C.c_void_p),
        ("lw_stride_obs", C.c_int64), ("lw_stride_draw", C.c_int64),
        ("mean", C.c_void_p), ("m2", C.c_void_p), ("pit_le", C.c_void_p), ("pit_lt", C.c_void_p), ("diag", C.c_void_p),
        ("elpd_i", C.c_void_p), ("n_replaced", C.c_void_p), ("n_pit_skipped", C.c_void_p),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(GlmPredictArgs)
        self.glm.struct_size = C.sizeof(GlmArgs)


class EngineError(RuntimeError):
    """A C-ABI call returned a negative status."""

    def __init__(self, code, msg):
        super().__init__(f"libpyloo_amd status {code}: {msg}")
        self.code = code


_lib = None


def load_library():
    """dlopen the in-tree library; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    from .build import LIB_PATH  # (imported here so that `python -m pyloo_amd.build` runs the module once)

    lib_path = os.environ.get("PYLOO_AMD_LIB", LIB_PATH)  # profiling builds (tools/ablate.sh)
    if not os.path.exists(lib_path):
        raise RuntimeError(
            f"{lib_path} is missing: the HIP engine has not been built "
            "(run `python -m pyloo_amd.build`).  pyloo_amd has no CPU fallback."
        )
    # PyTorch-ROCm wheels bundle their own HIP runtime (same SONAME libamdhip64.so.7).  Two HIP
    # runtimes in one process cannot both own the GPU, so torch must be loaded FIRST: our
    # library's NEEDED entry then binds to the runtime torch already mapped, and torch tensors,
    # streams and this engine share one HIP context.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for pure NumPy callers
        pass
    lib = C.CDLL(lib_path)
    i64, dbl, vp, ci = C.c_int64, C.c_double, C.c_void_p, C.c_int
    lib.pla_abi_version.restype = ci
    lib.pla_last_error.restype = C.c_char_p
    lib.pla_device_count.argtypes = [C.POINTER(ci)]
    lib.pla_engine_create.argtypes = [ci, C.POINTER(vp)]
    lib.pla_engine_destroy.argtypes = [vp]
    lib.pla_tail_count.argtypes = [i64, dbl, C.POINTER(i64)]
    lib.pla_psis_loo.argtypes = [vp, vp, ci, i64, i64, i64, i64, ci, i64, dbl, dbl, ci, vp, vp, vp, vp, vp]
    lib.pla_importance_weights.argtypes = [vp, vp, ci, i64, i64, i64, i64, ci, i64, ci, vp, vp, vp]
    lib.pla_reduce_pointwise.argtypes = [vp, vp, vp, vp, i64, dbl, ci, vp, vp]
    lib.pla_waic.argtypes = [vp, vp, ci, i64, i64, i64, i64, dbl, ci, vp, vp, vp, vp, vp]
    lib.pla_psis_loo_rows.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, i64, ci, i64, dbl, dbl, ci, vp, vp, vp, vp, vp]
    lib.pla_waic_rows.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, i64, dbl, ci, vp, vp, vp, vp, vp]
    lib.pla_e_loo.argtypes = [vp, vp, vp, vp, ci, i64, i64, i64, i64, i64, ci, vp, vp, vp, vp, vp, vp]
    lib.pla_e_loo_quantiles.argtypes = [vp, vp, vp, ci, i64, i64, i64, i64, vp, i64, ci, vp, vp]
    lib.pla_engine_set_frozen.argtypes = [vp, ci]
    lib.pla_engine_set_timing.argtypes = [vp, ci]
    lib.pla_engine_kernel_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    lib.pla_engine_first_kernel_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64)]
    lib.pla_fill_synthetic.argtypes = [vp, vp, ci, i64, i64, i64, C.c_uint64, dbl, dbl, dbl, dbl, vp]
    lib.pla_fill_synthetic_chains.argtypes = [vp, vp, ci, i64, i64, i64, C.c_uint64, ci, dbl, dbl, dbl, dbl, vp]
    lib.pla_engine_last_kernels.argtypes = [vp, C.c_char_p, ci]
    lib.pla_aggregate_pack.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.pla_aggregate_merge.argtypes = [vp, vp, ci, vp, vp]
    lib.pla_env_overrides.argtypes = [C.c_char_p, ci]
    lib.pla_engine_stream_stats.argtypes = [vp, C.POINTER(i64)]
    lib.pla_group_sum.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, vp, i64, ci, vp, vp, vp]
    lib.pla_psis_loo_groups.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, vp, i64, ci, i64, dbl, dbl, ci, vp, vp, vp, vp, vp, vp]
    lib.pla_compare_moments.argtypes = [vp, vp, ci, i64, i64, i64, i64, ci, vp, vp]
    lib.pla_stacking_eval.argtypes = [vp, vp, ci, i64, i64, i64, dbl, vp, ci, vp, vp]
    lib.pla_bb_bootstrap.argtypes = [vp, vp, ci, i64, i64, i64, dbl, i64, dbl, C.c_uint64, ci, vp, vp]
    lib.pla_bb_gamma_draws.argtypes = [vp, C.c_uint64, dbl, i64, i64, ci, vp, vp]
    lib.pla_engine_set_compare_grid.argtypes = [vp, ci]
    lib.pla_nonfactor_loglik.argtypes = [vp, vp, vp, vp, vp, ci, i64, i64, i64, i64, ci, ci, vp, vp, i64, i64, vp]
    lib.pla_engine_set_nonfactor_route.argtypes = [vp, ci]
    lib.pla_engine_set_nonfactor_grid.argtypes = [vp, ci]
    lib.pla_nonfactor_lds_max_obs.argtypes = []
    lib.pla_gather_draws.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, i64, ci, vp, vp, vp]
    lib.pla_psis_loo_draws.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, i64, ci, i64, dbl, dbl, ci, vp, vp, vp, vp, vp, vp]
    lib.pla_gather_lds_max_draws.argtypes = [ci]
    lib.pla_kfold_lme.argtypes = [vp, vp, vp, vp, vp, vp, i64, ci, ci, vp, vp, vp, i64, ci, vp, vp, i64, vp]
    lib.pla_kfold_reduce.argtypes = [vp, vp, vp, i64, dbl, vp, ci, vp, vp, vp, vp]
    lib.pla_mm_moments.argtypes = [vp, vp, vp, i64, i64, i64, ci, vp, vp, vp]
    lib.pla_mm_transform.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, vp, vp]
    lib.pla_mm_ratios.argtypes = [vp, ci, vp, vp, vp, vp, i64, i64, vp, vp]
    lib.pla_mixis_draw_lse.argtypes = [vp, vp, ci, i64, i64, i64, i64, ci, vp, vp, vp]
    lib.pla_mixis_loo.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, dbl, ci, vp, vp, vp]
    lib.pla_engine_set_mixis_grid.argtypes = [vp, ci]
    lib.pla_mixis_tile_rows.argtypes = [i64]
    lib.pla_loo_pit.argtypes = [vp, vp, vp, vp, ci, i64, i64, i64, i64, i64, i64, ci, ci, i64, ci, vp, vp, vp, vp, vp]
    lib.pla_loo_diag.argtypes = [vp, vp, ci, i64, i64, i64, i64, vp, i64, ci, i64, ci, vp, vp, vp, vp, vp, vp]
    lib.pla_loo_diag_weights.argtypes = [vp, vp, vp, ci, i64, i64, i64, i64, i64, i64, ci, vp, vp, vp, vp]
    lib.pla_loo_influence.argtypes = [C.POINTER(InfluenceArgs)]
    lib.pla_glm.argtypes = [C.POINTER(GlmArgs)]
    lib.pla_glm_grouped.argtypes = [C.POINTER(GlmGroupedArgs)]
    lib.pla_glm_marginal.argtypes = [C.POINTER(GlmMarginalArgs)]
    lib.pla_glm_marginal_segment.argtypes = []
    lib.pla_glm_predict.argtypes = [C.POINTER(GlmPredictArgs)]
    lib.pla_glm_predict_segment.argtypes = []
    lib.pla_lfo_ratios.argtypes = [vp, vp, ci, i64, i64, i64, i64, i64, i64, ci, vp, vp, vp]
    lib.pla_lfo.argtypes = [vp, vp, ci, i64, i64, i64, i64, i64, i64, i64, ci, i64, dbl, ci, vp, vp, vp, vp, vp]
    lib.pla_relative_eff.argtypes = [vp, vp, ci, i64, i64, i64, i64, i64, ci, ci, vp, vp, vp]
    lib.pla_engine_set_ess_grid.argtypes = [vp, ci]
    lib.pla_ess_lds_max_draws.argtypes = []
    for name in SYMBOLS:
        getattr(lib, name)  # AttributeError if the header and the library disagree
        if name != "pla_last_error":
            getattr(lib, name).restype = ci
    if lib.pla_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libpyloo_amd ABI {lib.pla_abi_version()} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise EngineError(code, load_library().pla_last_error().decode("utf-8", "replace"))


def env_overrides():
    """Run-time switches of the library that are set in the environment ("" when none is): ``pla_env_overrides``."""
    buf = C.create_string_buffer(1024)
    check(load_library().pla_env_overrides(buf, 1024))
    return buf.value.decode("utf-8", "replace")


def device_count():
    n = C.c_int(0)
    rc = load_library().pla_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def tail_count(n_draws, reff):
    out = C.c_int64(0)
    check(load_library().pla_tail_count(int(n_draws), float(reff), C.byref(out)))
    return out.value


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float64:
        return PLA_F64
    if dt == np.float32:
        return PLA_F32
    raise TypeError(f"unsupported dtype {dt}")

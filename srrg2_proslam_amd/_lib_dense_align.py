"""ctypes binding of include/proslam_hip_dense_align.h, the fifth public header of libproslam_hip.so (dense frame-to-model aligner).

The main header is pinned to the layout of PRS_ABI_VERSION 104, and with it _lib.SYMBOLS, _lib.STRUCT_SIZES and the mirrors of
_lib.py; what the fifth header declares is bound here, on the handle _lib.load() returns, until it joins the main header at the
next layout bump.  There is no CPU fallback: a library that does not export these symbols is an error.
"""
import ctypes as C

from . import _lib

_vp = C.c_void_p

SAMPLES_PER_THREAD = 4  # PRS_DENSE_ALIGN_SAMPLES_PER_THREAD


class DenseAlignParams(C.Structure):
    """prs_dense_align_params"""
    _fields_ = [("depth_type", C.c_int32), ("depth_scaling_factor_to_meters", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float), ("max_distance", C.c_float),
                ("min_normal_cos", C.c_float), ("robustifier", C.c_int32), ("chi_threshold", C.c_float), ("damping", C.c_float),
                ("max_iterations", C.c_int32), ("min_num_inliers", C.c_int32), ("linearize_only", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class DenseAlignResult(C.Structure):
    """prs_dense_align_result"""
    _fields_ = [("H", C.c_float * 36), ("b", C.c_float * 6), ("chi_inliers", C.c_float), ("chi_total", C.c_float),
                ("num_inliers", C.c_int32), ("num_outliers", C.c_int32), ("num_rejected", C.c_int32), ("num_invalid", C.c_int32),
                ("num_unmatched", C.c_int32), ("num_samples", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32),
                ("steps_taken", C.c_int32), ("warnings", C.c_int32), ("reserved", C.c_int32 * 2)]


class DenseAlignBatch(C.Structure):
    """prs_dense_align_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("step", C.c_int32), ("model_pitch", C.c_int32),
                ("live_pitch", C.c_int32), ("reserved0", C.c_int32 * 2), ("model_depth", C.c_void_p), ("model_normal", C.c_void_p),
                ("live_depth", C.c_void_p), ("live_normal", C.c_void_p), ("X", C.c_void_p), ("result", C.c_void_p),
                ("mask", C.c_void_p), ("workspace", C.c_void_p), ("reserved", C.c_void_p * 2)]


# every symbol include/proslam_hip_dense_align.h declares: (restype, argtypes)
SYMBOLS = {
    "prs_dense_align_batch_run": (C.c_int, [_vp, C.POINTER(DenseAlignParams), C.POINTER(DenseAlignBatch)]),
    "prs_dense_align_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_dense_align_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
}

# every *_struct_sizes entry with the mirrors of the structs it reports, in the order its function writes them
STRUCT_SIZES = (
    ("prs_dense_align_struct_sizes", (DenseAlignParams, DenseAlignBatch, DenseAlignResult)),
)

_bound = None


def load():
    """the library of _lib.load() with the symbols of the fifth header bound and its struct sizes compared; raises if the library
    is absent, older than the header or laid out differently"""
    global _bound
    if _bound is not None:
        return _bound
    lib = _lib.load()
    for name, (restype, argtypes) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("libproslam_hip.so does not export %s: rebuild with `python -c 'import __graft_entry__ as g; g.build()'`"
                              % name)
        fn.restype = restype
        fn.argtypes = argtypes
    for query, mirrors in STRUCT_SIZES:
        sizes = (C.c_uint64 * len(mirrors))()
        getattr(lib, query)(sizes)
        mine = [C.sizeof(m) for m in mirrors]
        if list(sizes) != mine:
            raise ImportError("libproslam_hip.so lays out %s as %s bytes, the Python binding as %s: rebuild with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`"
                              % (" / ".join(_lib.c_name(m) for m in mirrors), list(sizes), mine))
    _bound = lib
    return lib

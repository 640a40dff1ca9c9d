"""ctypes binding of include/proslam_hip_tsdf_mesh.h, the sixth public header of libproslam_hip.so (TSDF mesh).

The main header is pinned to the layout of PRS_ABI_VERSION 104, and with it _lib.SYMBOLS, _lib.STRUCT_SIZES and the mirrors of
_lib.py; what the sixth header declares is bound here, on the handle _lib.load() returns, until it joins the main header at the
next layout bump.  The call takes the prs_tsdf_params of the third header (_lib_tsdf.TsdfParams).  There is no CPU fallback: a
library that does not export these symbols is an error.
"""
import ctypes as C

from . import _lib, _lib_tsdf

_vp = C.c_void_p


class TsdfMeshBatch(C.Structure):
    """prs_tsdf_mesh_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("vertex_stride", C.c_int32),
                ("quad_stride", C.c_int32), ("origin", C.c_void_p), ("volume", C.c_void_p), ("vertex", C.c_void_p),
                ("normal", C.c_void_p), ("quad", C.c_void_p), ("cube", C.c_void_p), ("edge", C.c_void_p), ("n_vertices", C.c_void_p),
                ("n_vertices_total", C.c_void_p), ("n_quads", C.c_void_p), ("n_quads_total", C.c_void_p), ("status", C.c_void_p),
                ("workspace", C.c_void_p), ("reserved", C.c_void_p * 3)]


# every symbol include/proslam_hip_tsdf_mesh.h declares: (restype, argtypes)
SYMBOLS = {
    "prs_tsdf_mesh_batch_run": (C.c_int, [_vp, C.POINTER(_lib_tsdf.TsdfParams), C.POINTER(TsdfMeshBatch)]),
    "prs_tsdf_mesh_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_tsdf_mesh_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
}

# every *_struct_sizes entry with the mirrors of the structs it reports, in the order its function writes them
STRUCT_SIZES = (
    ("prs_tsdf_mesh_struct_sizes", (TsdfMeshBatch,)),
)

_bound = None


def load():
    """the library of _lib.load() with the symbols of the sixth header bound and its struct sizes compared; raises if the library
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

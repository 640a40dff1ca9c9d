"""The whole C-ABI boundary, derived from include/proslam_hip.h as the C compiler lays it out (tests/abi_probe.py): the header against
the pinned layout of its version, the ctypes mirrors and the SYMBOLS table of srrg2_proslam_amd/_lib.py against the header, the built
library against both, and the constants the Python package restates.  No GPU needed."""
import ctypes as C
import json
import keyword
import os
import re

import pytest

import abi_probe
from srrg2_proslam_amd import _lib

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_v104.json")
# header structs without a ctypes mirror: rows of arrays that cross the boundary as numpy arrays, never built field by field
ARRAY_ROWS = {
    "prs_corr": "rows of the correspondence arrays; ops.CORR_DTYPE",
    "prs_kp2": "rows of (n, 2) float32 keypoint arrays",
    "prs_camera_measurement": "rows of the map's measurement arrays, passed as (n, 3) float32 plus a frame index",
    "prs_frame_pose": "rows of the map's pose arrays, passed as (n, 16) float32",
}
MIRRORS = [m for m in vars(_lib).values() if isinstance(m, type) and issubclass(m, C.Structure) and m is not C.Structure]


@pytest.fixture(scope="module")
def header():
    return abi_probe.snapshot()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def c_field(name):
    """a mirror names a field as the header does; where that is a Python keyword it appends one underscore (lambda_, from_)"""
    return name[:-1] if name.endswith("_") and keyword.iskeyword(name[:-1]) else name


# ---- header against pin ----

def test_header_is_the_pinned_layout(header):
    pin = json.load(open(PIN))
    hint = ": a layout change needs a PRS_ABI_VERSION bump and a new pin (python tests/abi_probe.py > tests/golden/abi_v<N>.json)"
    assert header["constants"]["PRS_ABI_VERSION"] == 104 == _lib.ABI_VERSION, "the pin is version 104's" + hint
    for section in ("structs", "constants", "prototypes"):
        assert list(header[section]) == list(pin[section]), "%s added, removed or reordered%s" % (section, hint)
        for name, value in header[section].items():
            assert value == pin[section][name], "%s changed: %s, pinned %s%s" % (name, value, pin[section][name], hint)
    assert open(PIN).read() == abi_probe.dumps(header)
    assert len(header["structs"]) == 72 and len(header["prototypes"]) == 139


# ---- mirrors against compiled header ----

def test_every_struct_is_mirrored_or_an_array_row(header):
    named = [_lib.c_name(m) for m in MIRRORS]
    assert len(set(named)) == len(named), "two mirrors name one struct"
    assert set(named) <= set(header["structs"]), "mirrors of no header struct: %s" % sorted(set(named) - set(header["structs"]))
    assert set(header["structs"]) - set(named) == set(ARRAY_ROWS)


def test_mirror_has_the_header_layout(header):
    assert len(MIRRORS) == 68
    wrong = []
    for mirror in MIRRORS:
        size, fields = header["structs"][_lib.c_name(mirror)]
        mine = [[c_field(n), getattr(mirror, n).offset, getattr(mirror, n).size] for n, *_ in mirror._fields_]
        if C.sizeof(mirror) != size:
            wrong.append("%s: %d bytes, %s has %d" % (mirror.__name__, C.sizeof(mirror), _lib.c_name(mirror), size))
        wrong += ["%s: field %d is %s, the header's %s" % (mirror.__name__, i, a, b) for i, (a, b) in enumerate(zip(mine, fields)) if a != b]
        if len(mine) != len(fields):
            wrong.append("%s: %d fields, the header's %d" % (mirror.__name__, len(mine), len(fields)))
    assert not wrong, "\n".join(wrong)


def test_numpy_rows_have_the_header_layout(header):
    from srrg2_proslam_amd import ops
    for dtype, struct in ((ops.CORR_DTYPE, "prs_corr"), (ops._TRAJ_RESULT_DTYPE, "prs_trajectory_result")):
        size, fields = header["structs"][struct]
        assert dtype.itemsize == size
        assert [[n, dtype.fields[n][1], dtype.fields[n][0].itemsize] for n in dtype.names] == fields, struct
    assert [str(ops.CORR_DTYPE[n]) for n in ops.CORR_DTYPE.names] == ["int32", "int32", "float32"]


# ---- SYMBOLS against prototypes ----

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double, "uint8_t": C.c_uint8, "char": C.c_char}


def scalar_kind(ct):
    """(width, float or integer, signed): what decides how a scalar crosses the boundary; int and int32_t are one kind"""
    return C.sizeof(ct), ct._type_ in "fdg", ct._type_ in "fdg" or ct._type_.islower()


def bound_as(c_type, bound):
    """None when ctypes type `bound` passes C type `c_type` faithfully, else what is wrong with it"""
    if c_type == "void":
        return None if bound is None else "void bound as %s" % bound
    if bound is None:
        return "%s bound as None" % c_type
    if not c_type.endswith("*"):
        if not (isinstance(bound, type) and issubclass(bound, C._SimpleCData)) or bound in (C.c_void_p, C.c_char_p):
            return "scalar %s bound as %s" % (c_type, bound.__name__)
        return None if scalar_kind(bound) == scalar_kind(SCALARS[c_type]) else "%s bound as %s" % (c_type, bound.__name__)
    pointee = c_type[:-1].replace("const ", "")
    if bound is C.c_void_p:
        return None  # an address: a device pointer, a handle or a numpy buffer
    if bound is C.c_char_p:
        return None if pointee == "char" else "%s bound as c_char_p" % c_type
    if not issubclass(bound, C._Pointer):
        return "pointer %s bound as %s" % (c_type, bound.__name__)
    target = bound._type_
    if issubclass(target, C.Structure):
        return None if _lib.c_name(target) == pointee else "%s bound as POINTER(%s)" % (c_type, target.__name__)
    if pointee.endswith("*") or pointee not in SCALARS:  # prs_context**: the address of a handle
        return None if target is C.c_void_p else "%s bound as POINTER(%s)" % (c_type, target.__name__)
    return None if scalar_kind(target) == scalar_kind(SCALARS[pointee]) else "%s bound as POINTER(%s)" % (c_type, target.__name__)


def test_symbols_are_the_header_prototypes(header):
    protos = header["prototypes"]
    assert sorted(_lib.SYMBOLS) == sorted(protos)
    wrong = []
    for name, (restype, argtypes) in _lib.SYMBOLS.items():
        ret, params = protos[name]
        if len(argtypes) != len(params):
            wrong.append("%s: %d arguments bound, %d declared" % (name, len(argtypes), len(params)))
            continue
        for where, c_type, bound in [("returns", ret, restype)] + [("argument %d" % i, p, a) for i, (p, a) in enumerate(zip(params, argtypes))]:
            why = bound_as(c_type, bound)
            if why:
                wrong.append("%s %s: %s" % (name, where, why))
    assert not wrong, "\n".join(wrong)


def test_bound_as_refuses_what_ctypes_would_truncate():
    assert bound_as("uint64_t", C.c_uint64) is None and bound_as("int", C.c_int32) is None and bound_as("const char*", C.c_char_p) is None
    assert bound_as("const prs_pcf_params*", C.POINTER(_lib.PcfParams)) is None and bound_as("prs_map**", C.POINTER(C.c_void_p)) is None
    for c_type, bound in (("uint64_t", C.c_int), ("uint64_t", C.c_int64), ("int64_t", C.c_int32), ("float", C.c_double), ("float", C.c_int32),
                          ("int32_t", C.c_void_p), ("const float*", C.c_int64), ("int32_t*", C.POINTER(C.c_int64)), ("void", C.c_int),
                          ("int", None), ("const prs_pcf_params*", C.POINTER(_lib.PcfState)), ("prs_map**", C.POINTER(C.c_int32))):
        assert bound_as(c_type, bound), (c_type, bound)


# ---- library against header ----

def test_library_exports_every_prototype(header, built):
    raw = C.CDLL(_lib.LIB_PATH)
    missing = [n for n in header["prototypes"] if not hasattr(raw, n)]
    assert not missing, "declared in include/proslam_hip.h but not exported: %s" % missing
    assert built.prs_version() == header["constants"]["PRS_ABI_VERSION"]


def test_struct_sizes_entries_report_the_compiled_sizes(header, built):
    table = dict(_lib.STRUCT_SIZES)
    assert sorted(table) == sorted(n for n in header["prototypes"] if n.endswith("_struct_sizes")) and len(table) == len(_lib.STRUCT_SIZES)
    for query, mirrors in table.items():
        # the header names the parameter after the count it writes: "uint64_t* sizes3"
        count = int(re.search(r"\b%s\(uint64_t\* sizes(\d+)\)" % query, abi_probe.header_text()).group(1))
        assert len(mirrors) == count, query
        sizes = (C.c_uint64 * count)()
        getattr(built, query)(sizes)
        assert list(sizes) == [header["structs"][_lib.c_name(m)][0] for m in mirrors], query


# ---- constants ----

def test_restated_constants_have_the_header_values(header):
    from srrg2_proslam_amd import ops
    constants, checked = header["constants"], set()
    for module in (_lib, ops):
        for name, value in vars(module).items():
            if name.isupper() and isinstance(value, int) and "PRS_" + name in constants:
                assert value == constants["PRS_" + name], "%s.%s" % (module.__name__, name)
                checked.add(name)
    # the rule finds what it is meant to find: the status codes, the version and each stage's enumerators
    assert {"OK", "WARN_SPARSE_DEPTH", "ERR_NULL", "ERR_NO_DEVICE", "ERR_NOT_POSITIVE_DEFINITE", "ABI_VERSION", "POSE_GRAPH_MAX_ITERATIONS",
            "DAMPING_IDENTITY", "CLOSURE_UVD", "SESSION_SPLIT_LOST", "TRAJ_ALIGN_RIGID", "DISPATCH_MERGE", "DEPTH_F32", "PIXEL_F32",
            "RECTIFY_NEAREST", "VOXEL_MEAN", "DISTORTION_RADTAN", "MERGER_DEPTH_EKF", "SELECT_LIBSTDCXX"} <= checked

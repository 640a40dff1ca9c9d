"""The fifth public header, include/proslam_hip_dense_align.h, as the C compiler lays it out against its binding
srrg2_proslam_amd/_lib_dense_align.py and the built library: what tests/test_tsdf_raycast_abi.py does for the fourth header, with the
same helpers (tests/abi_probe.py).  Also the params helper, the null-context refusal, the workspace query and what the header says it
leaves out.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import abi_probe
import dense_align_ref
import test_abi_layout as layout
from srrg2_proslam_amd import _lib, _lib_dense_align, _lib_normals, _lib_tsdf, _lib_tsdf_raycast

HEADER = os.path.join(abi_probe.ROOT, "include", "proslam_hip_dense_align.h")
MIRRORS = [m for m in vars(_lib_dense_align).values() if isinstance(m, type) and issubclass(m, C.Structure) and m is not C.Structure]
STRUCTS = ["prs_dense_align_params", "prs_dense_align_result", "prs_dense_align_batch"]
ENTRIES = ["prs_dense_align_batch_run", "prs_dense_align_workspace_bytes", "prs_dense_align_struct_sizes"]
CONSTANTS = ("PRS_ABI_VERSION", "PRS_DEPTH_U16", "PRS_DEPTH_F32", "PRS_ROBUSTIFIER_CLAMP", "PRS_ROBUSTIFIER_SATURATED", "PRS_OK",
             "PRS_ERR_NULL", "PRS_ERR_RANGE", "PRS_ERR_UNSUPPORTED", "PRS_DENSE_ALIGN_SAMPLES_PER_THREAD")


def header_text():
    return open(HEADER).read()


@pytest.fixture(scope="module")
def probe():
    """{"structs": {name: [size, [[field, offset, size], ...]]}, "prototypes": {...}, "constants": the main header's constants as this
    header sees them, and its own one} from a C program that includes the fifth header alone"""
    text = header_text()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "proslam_hip_dense_align.h"', "int main(void) {"]
    for struct, fields in abi_probe._declared(text):
        lines.append('  printf("S %s %%lu\\n", (unsigned long) sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('  printf("F %s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s*) 0)->%s));'
                         % (f, struct, f, struct, f))
    for c in CONSTANTS:
        lines.append('  printf("C %s %%lld\\n", (long long) (%s));' % (c, c))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write("\n".join(lines + ["  return 0;", "}", ""]))
        subprocess.run(abi_probe.compiler() + ["-x", "c", "-std=c99", "-Wall", "-pedantic", "-I", os.path.dirname(HEADER), src, "-o", exe],
                       check=True)
        printed = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    structs, constants = {}, {}
    for tag, name, *numbers in (line.split() for line in printed.splitlines()):
        if tag == "S":
            fields = structs[name] = [int(numbers[0]), []]
        elif tag == "F":
            fields[1].append([name, int(numbers[0]), int(numbers[1])])
        else:
            constants[name] = int(numbers[0])
    return {"structs": structs, "prototypes": abi_probe.prototypes(text), "constants": constants}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return _lib_dense_align.load()


def test_the_header_adds_to_the_main_header_and_does_not_restate_it(probe):
    text = header_text()
    assert '#include "proslam_hip.h"' in text and "joins it" in text.split("#ifndef")[0]
    assert "at the next layout bump" in " ".join(text.split("#ifndef")[0].replace("\n *", " ").split())
    assert abi_probe._constant_names(text) == ["PRS_DENSE_ALIGN_SAMPLES_PER_THREAD"]      # the one constant of its own: the rule's P
    assert probe["constants"] == dict(PRS_ABI_VERSION=104, PRS_DEPTH_U16=0, PRS_DEPTH_F32=1, PRS_ROBUSTIFIER_CLAMP=0,
                                      PRS_ROBUSTIFIER_SATURATED=1, PRS_OK=0, PRS_ERR_NULL=-1, PRS_ERR_RANGE=-4, PRS_ERR_UNSUPPORTED=-5,
                                      PRS_DENSE_ALIGN_SAMPLES_PER_THREAD=4)
    assert probe["constants"]["PRS_DENSE_ALIGN_SAMPLES_PER_THREAD"] == dense_align_ref.P == _lib_dense_align.SAMPLES_PER_THREAD
    assert list(probe["structs"]) == STRUCTS and list(probe["prototypes"]) == ENTRIES
    main = abi_probe.snapshot()
    assert not set(probe["structs"]) & set(main["structs"]) and not set(probe["prototypes"]) & set(main["prototypes"])
    assert "PRS_DENSE_ALIGN_SAMPLES_PER_THREAD" not in main["constants"]
    assert [probe["structs"][s][0] for s in STRUCTS] == [80, 224, 112]
    for name in probe["structs"]:                                       # every one ends in reserved words
        assert probe["structs"][name][1][-1][0] == "reserved", name
    mine = [f[0] for f in probe["structs"]["prs_dense_align_params"][1]]
    assert mine == ["depth_type", "depth_scaling_factor_to_meters", "fx", "fy", "cx", "cy", "range_min", "range_max", "max_distance",
                    "min_normal_cos", "robustifier", "chi_threshold", "damping", "max_iterations", "min_num_inliers", "linearize_only",
                    "reserved"]
    # the fields the point aligner's parameters and result share keep their names
    shared = {n for n, *_ in _lib.PointAlignParams._fields_} & set(mine)
    assert shared >= {"robustifier", "chi_threshold", "damping", "max_iterations", "min_num_inliers", "linearize_only"}
    result = [f[0] for f in probe["structs"]["prs_dense_align_result"][1]]
    assert result == ["H", "b", "chi_inliers", "chi_total", "num_inliers", "num_outliers", "num_rejected", "num_invalid", "num_unmatched",
                      "num_samples", "status", "iterations", "steps_taken", "warnings", "reserved"]
    assert tuple(result[:-1]) == dense_align_ref.RESULT_FIELDS
    batch = [f[0] for f in probe["structs"]["prs_dense_align_batch"][1]]
    assert batch == ["batch", "rows", "cols", "step", "model_pitch", "live_pitch", "reserved0", "model_depth", "model_normal", "live_depth",
                     "live_normal", "X", "result", "mask", "workspace", "reserved"]


def test_mirrors_have_the_header_layout(probe):
    assert sorted(_lib.c_name(m) for m in MIRRORS) == sorted(probe["structs"])
    for mirror in MIRRORS:
        size, fields = probe["structs"][_lib.c_name(mirror)]
        mine = [[layout.c_field(n), getattr(mirror, n).offset, getattr(mirror, n).size] for n, *_ in mirror._fields_]
        assert C.sizeof(mirror) == size and mine == fields, mirror.__name__


def test_the_result_dtype_of_ops_has_the_header_layout(probe):
    from srrg2_proslam_amd import ops
    size, fields = probe["structs"]["prs_dense_align_result"]
    dt = ops.DENSE_ALIGN_RESULT_DTYPE
    assert dt.itemsize == size
    assert [[n, dt.fields[n][1], dt.fields[n][0].itemsize] for n in dt.names] == fields


def test_the_five_bindings_have_no_symbol_in_common():
    names = [set(_lib.SYMBOLS), set(_lib_normals.SYMBOLS), set(_lib_tsdf.SYMBOLS), set(_lib_tsdf_raycast.SYMBOLS),
             set(_lib_dense_align.SYMBOLS)]
    for i in range(5):
        for j in range(i + 1, 5):
            assert not names[i] & names[j], (i, j)
    others = list(vars(_lib).values()) + list(vars(_lib_normals).values()) + list(vars(_lib_tsdf).values()) + \
        list(vars(_lib_tsdf_raycast).values())
    assert not [m for m in others if isinstance(m, type) and issubclass(m, C.Structure) and m.__module__.endswith("_lib_dense_align")]
    assert _lib.ABI_VERSION == 104


def test_bindings_match_the_prototypes(probe):
    assert sorted(_lib_dense_align.SYMBOLS) == sorted(probe["prototypes"])
    wrong = []
    for name, (restype, argtypes) in _lib_dense_align.SYMBOLS.items():
        ret, params = probe["prototypes"][name]
        assert len(argtypes) == len(params), name
        for where, c_type, bound in [("returns", ret, restype)] + [("argument %d" % i, p, a) for i, (p, a) in enumerate(zip(params, argtypes))]:
            why = layout.bound_as(c_type, bound)
            if why:
                wrong.append("%s %s: %s" % (name, where, why))
    assert not wrong, "\n".join(wrong)


def test_library_exports_the_symbols_and_reports_the_compiled_sizes(probe, built):
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in probe["prototypes"])
    assert built.prs_version() == 104
    table = dict(_lib_dense_align.STRUCT_SIZES)
    assert sorted(table) == sorted(n for n in probe["prototypes"] if n.endswith("_struct_sizes"))
    for query, mirrors in table.items():
        count = int(re.search(r"\b%s\(uint64_t\* sizes(\d+)\)" % query, header_text()).group(1))
        assert len(mirrors) == count == 3
        sizes = (C.c_uint64 * count)()
        getattr(built, query)(sizes)
        assert list(sizes) == [probe["structs"][_lib.c_name(m)][0] for m in mirrors]


def test_workspace_query(built):
    q = built.prs_dense_align_workspace_bytes
    P = dense_align_ref.P
    record, chunk = 128, 256 * P
    assert q(1, 1, 1, 1) == 16 + record
    assert q(1, 32, 32, 1) == 16 + -(-1024 // chunk) * record and q(1, 41, 25, 1) == 16 + -(-1025 // chunk) * record
    assert q(3, 480, 640, 1) == 16 + 3 * -(-307200 // chunk) * record
    assert q(5, 480, 640, 4) == 32 + 5 * -(-(120 * 160) // chunk) * record
    assert q(5, 481, 641, 4) == 32 + 5 * -(-(121 * 161) // chunk) * record
    for refused in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (-1, 4, 4, 1), (1, 4, 4, -2)):
        assert q(*refused) == 0, refused
    assert q(1, 1 << 16, 1 << 15, 1) == 0                                # rows * cols beyond 2^31 - 1
    assert q(1, 1 << 16, (1 << 15) - 1, 1 << 14) > 0
    chunks = -(-307200 // chunk)
    assert q((1 << 31) // chunks + 1, 480, 640, 1) == 0                  # batch * chunks beyond 2^31 - 1
    assert q(((1 << 31) - 1) // chunks, 480, 640, 1) > 0


def test_header_says_what_the_stage_leaves_out():
    text = header_text()
    section = " ".join(text[text.index(" * Dense align:"):text.index("} prs_dense_align_params;")].replace("\n *", " ").split())
    for left_out in ("a colour / photometric term", "an image pyramid", "bilateral pre-filtering", "a termination criterion",
                     "host-pointer variant", "C++ adapter in plugin/"):
        assert left_out in section, left_out
    for stated in ("((W0 + W1) + W2) + W3", "m = 32, 16, 8, 4, 2, 1", "chunk q / (256 * P)", "ascending c", "X <- X exp(dx)"):
        assert stated in section, stated


def test_null_context_is_refused(built):
    p, o = _lib_dense_align.DenseAlignParams(), _lib_dense_align.DenseAlignBatch()
    assert built.prs_dense_align_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL
    assert built.prs_dense_align_batch_run(None, None, None) == -1


def test_params_helper_and_config(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.DenseAlignBatch) and callable(ops.DenseTrackerBatch)
    cam = dict(fx=481.2, fy=-480.0, cx=319.5, cy=239.5)
    p = ops.dense_align_params(cam)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert (p.depth_type, p.depth_scaling_factor_to_meters, p.robustifier) == (0, 1.0, 1)
    assert (p.max_distance, p.min_normal_cos, p.chi_threshold, p.damping) == (f32(0.2), f32(0.8), f32(0.01), 0.0)
    assert (p.max_iterations, p.min_num_inliers, p.linearize_only, p.range_min, p.range_max) == (10, 100, 0, f32(0.1), 10.0)
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(481.2), -480.0, 319.5, 239.5) and list(p.reserved) == [0] * 4
    cfg = configs.DENSE_ALIGN
    assert cfg == dict(max_distance=0.2, min_normal_cos=0.8, robustifier="saturated", chi_threshold=0.01, damping=0.0,
                       min_num_inliers=100, range_min=0.1, range_max=10.0, schedule=[(4, 4), (2, 5), (1, 10)])
    assert bytes(ops.dense_align_params(cam, **{k: v for k, v in cfg.items() if k != "schedule"})) == bytes(p)
    assert [s for s, _ in cfg["schedule"]] == sorted((s for s, _ in cfg["schedule"]), reverse=True) and cfg["schedule"][-1][0] == 1
    q = ops.dense_align_params(cam, "f32", 0.5, robustifier="clamp", max_iterations=0, linearize_only=1)
    assert (q.depth_type, q.depth_scaling_factor_to_meters, q.robustifier, q.max_iterations, q.linearize_only) == (1, 0.5, 0, 0, 1)
    rp = dense_align_ref.params(cam)
    assert all(float(rp[k]) == getattr(p, k) for k in ("max_distance", "min_normal_cos", "chi_threshold", "damping", "range_min", "range_max"))
    assert (rp["robustifier"], rp["max_iterations"], rp["min_num_inliers"]) == (p.robustifier, p.max_iterations, p.min_num_inliers)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=1e-50), dict(max_distance=0.0), dict(max_distance=inf),
                dict(max_distance=1e39), dict(min_normal_cos=1.5), dict(min_normal_cos=-1.01), dict(min_normal_cos=nan),
                dict(chi_threshold=-1e-3), dict(chi_threshold=nan), dict(damping=-0.1), dict(damping=inf), dict(range_min=-0.1),
                dict(range_min=2.0, range_max=1.0), dict(range_max=inf), dict(robustifier="huber"), dict(robustifier=2),
                dict(max_iterations=-1), dict(max_iterations=0), dict(depth_type="u8"), dict(depth_type=7)):
        with pytest.raises(ValueError):
            ops.dense_align_params(cam, **bad)
    with pytest.raises(ValueError):
        ops.dense_align_params(dict(cam, fx=nan))

"""The fourth public header, include/proslam_hip_tsdf_raycast.h, as the C compiler lays it out against its binding
srrg2_proslam_amd/_lib_tsdf_raycast.py and the built library: what tests/test_tsdf_abi.py does for the third header, with the same
helpers (tests/abi_probe.py).  Also the params helper, the null-context refusal, the workspace query and what the header says it
leaves out.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import abi_probe
import test_abi_layout as layout
from srrg2_proslam_amd import _lib, _lib_normals, _lib_tsdf, _lib_tsdf_raycast

HEADER = os.path.join(abi_probe.ROOT, "include", "proslam_hip_tsdf_raycast.h")
MIRRORS = [m for m in vars(_lib_tsdf_raycast).values() if isinstance(m, type) and issubclass(m, C.Structure) and m is not C.Structure]
STRUCTS = ["prs_tsdf_raycast_params", "prs_tsdf_raycast_batch"]
ENTRIES = ["prs_tsdf_raycast_batch_run", "prs_tsdf_raycast_workspace_bytes", "prs_tsdf_raycast_struct_sizes"]


def header_text():
    return open(HEADER).read()


@pytest.fixture(scope="module")
def probe():
    """{"structs": {name: [size, [[field, offset, size], ...]]}, "prototypes": {...}, "main": the main header's constants as this
    header sees them} from a C program that includes the fourth header alone"""
    text = header_text()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "proslam_hip_tsdf_raycast.h"', "int main(void) {"]
    for struct, fields in abi_probe._declared(text):
        lines.append('  printf("S %s %%lu\\n", (unsigned long) sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('  printf("F %s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s*) 0)->%s));'
                         % (f, struct, f, struct, f))
    for c in ("PRS_ABI_VERSION", "PRS_DEPTH_F32", "PRS_OK", "PRS_ERR_NULL", "PRS_ERR_RANGE", "PRS_ERR_UNSUPPORTED"):
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
    return {"structs": structs, "prototypes": abi_probe.prototypes(text), "main": constants}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return _lib_tsdf_raycast.load()


def test_the_header_adds_to_the_main_header_and_does_not_restate_it(probe):
    text = header_text()
    assert '#include "proslam_hip.h"' in text and "joins it" in text.split("#ifndef")[0]
    assert "at the next layout bump" in " ".join(text.split("#ifndef")[0].replace("\n *", " ").split())
    assert abi_probe._constant_names(text) == []                       # no constant of its own: the main header's are used
    assert probe["main"] == dict(PRS_ABI_VERSION=104, PRS_DEPTH_F32=1, PRS_OK=0, PRS_ERR_NULL=-1, PRS_ERR_RANGE=-4, PRS_ERR_UNSUPPORTED=-5)
    assert list(probe["structs"]) == STRUCTS and list(probe["prototypes"]) == ENTRIES
    main = abi_probe.snapshot()
    assert not set(probe["structs"]) & set(main["structs"]) and not set(probe["prototypes"]) & set(main["prototypes"])
    assert [probe["structs"][s][0] for s in STRUCTS] == [112, 144]
    for name in probe["structs"]:                                       # every one ends in reserved words
        assert probe["structs"][name][1][-1][0] == "reserved", name
    # the fields the TSDF calls share keep their names
    mine = [f[0] for f in probe["structs"]["prs_tsdf_raycast_params"][1]]
    assert mine == ["fx", "fy", "cx", "cy", "range_min", "range_max", "sensor_in_robot", "voxel_size", "min_weight", "step", "reserved"]
    assert set(mine[:9]) <= set(n for n, *_ in _lib_tsdf.TsdfParams._fields_)
    batch = [f[0] for f in probe["structs"]["prs_tsdf_raycast_batch"][1]]
    assert batch == ["batch", "views", "rows", "cols", "pitch", "pose_stride", "nx", "ny", "nz", "reserved0", "origin", "volume", "pose",
                     "view_index", "n_views", "depth", "normal", "n_hit", "n_skipped", "status", "workspace", "reserved"]


def test_mirrors_have_the_header_layout(probe):
    assert sorted(_lib.c_name(m) for m in MIRRORS) == sorted(probe["structs"])
    for mirror in MIRRORS:
        size, fields = probe["structs"][_lib.c_name(mirror)]
        mine = [[layout.c_field(n), getattr(mirror, n).offset, getattr(mirror, n).size] for n, *_ in mirror._fields_]
        assert C.sizeof(mirror) == size and mine == fields, mirror.__name__


def test_the_four_bindings_have_no_symbol_in_common():
    names = [set(_lib.SYMBOLS), set(_lib_normals.SYMBOLS), set(_lib_tsdf.SYMBOLS), set(_lib_tsdf_raycast.SYMBOLS)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not names[i] & names[j], (i, j)
    others = list(vars(_lib).values()) + list(vars(_lib_normals).values()) + list(vars(_lib_tsdf).values())
    assert not [m for m in others if isinstance(m, type) and issubclass(m, C.Structure) and m.__module__.endswith("_lib_tsdf_raycast")]
    assert _lib.ABI_VERSION == 104


def test_bindings_match_the_prototypes(probe):
    assert sorted(_lib_tsdf_raycast.SYMBOLS) == sorted(probe["prototypes"])
    wrong = []
    for name, (restype, argtypes) in _lib_tsdf_raycast.SYMBOLS.items():
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
    table = dict(_lib_tsdf_raycast.STRUCT_SIZES)
    assert sorted(table) == sorted(n for n in probe["prototypes"] if n.endswith("_struct_sizes"))
    for query, mirrors in table.items():
        count = int(re.search(r"\b%s\(uint64_t\* sizes(\d+)\)" % query, header_text()).group(1))
        assert len(mirrors) == count == 2
        sizes = (C.c_uint64 * count)()
        getattr(built, query)(sizes)
        assert list(sizes) == [probe["structs"][_lib.c_name(m)][0] for m in mirrors]


def test_workspace_query(built):
    assert built.prs_tsdf_raycast_workspace_bytes(3, 5) == 3 * 5 * 64
    assert built.prs_tsdf_raycast_workspace_bytes(1, 1) == 64
    assert built.prs_tsdf_raycast_workspace_bytes(0, 5) == 0 and built.prs_tsdf_raycast_workspace_bytes(3, 0) == 0
    assert built.prs_tsdf_raycast_workspace_bytes(-1, 5) == 0 and built.prs_tsdf_raycast_workspace_bytes(3, -2) == 0
    assert built.prs_tsdf_raycast_workspace_bytes(1 << 16, 1 << 15) == 0                       # batch * views beyond 2^31 - 1
    assert built.prs_tsdf_raycast_workspace_bytes(1 << 16, (1 << 15) - 1) == ((1 << 31) - (1 << 16)) * 64


def test_header_says_what_the_stage_leaves_out():
    text = header_text()
    section = " ".join(text[text.index(" * TSDF raycast:"):text.index("} prs_tsdf_raycast_params;")].replace("\n *", " ").split())
    for left_out in ("empty-space skipping and adaptive steps", "a vertex image", "colour", "ray-length rather than z parameterisation",
                     "host-pointer variant", "C++ adapter in plugin/", "A surface thinner than `step` can be stepped over"):
        assert left_out in section, left_out
    # the fusion's header lists what it leaves out and does not name the raycast: this header is where it is declared
    assert "raycast" not in open(os.path.join(abi_probe.ROOT, "include", "proslam_hip_tsdf.h")).read()


def test_null_context_is_refused(built):
    p, o = _lib_tsdf_raycast.TsdfRaycastParams(), _lib_tsdf_raycast.TsdfRaycastBatch()
    assert built.prs_tsdf_raycast_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL
    assert built.prs_tsdf_raycast_batch_run(None, None, None) == -1


def test_params_helper_and_config(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.TsdfRaycastBatch)
    cam = dict(fx=481.2, fy=-480.0, cx=319.5, cy=239.5)
    p = ops.tsdf_raycast_params(cam)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert (p.voxel_size, p.step, p.min_weight, p.range_min, p.range_max) == (f32(0.02), f32(0.02), 1.0, f32(0.1), 10.0)
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(481.2), -480.0, 319.5, 239.5)
    assert list(p.sensor_in_robot) == list(np.eye(4).reshape(16)) and list(p.reserved) == [0] * 3
    assert configs.TSDF_RAYCAST == dict(step=0.02, min_weight=1.0, range_min=0.1, range_max=10.0)
    assert configs.TSDF_RAYCAST["step"] == configs.TSDF["voxel_size"] == configs.TSDF["truncation"] / 4
    assert bytes(ops.tsdf_raycast_params(cam, configs.TSDF["voxel_size"], **configs.TSDF_RAYCAST)) == bytes(p)
    S = np.arange(16, dtype=np.float32).reshape(4, 4)
    q = ops.tsdf_raycast_params(cam, 0.5, 1.5, -2, 0.0, 0.0, S)
    assert (q.voxel_size, q.step, q.min_weight, q.range_min, q.range_max) == (0.5, 1.5, -2.0, 0.0, 0.0)
    assert list(q.sensor_in_robot) == list(range(16))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(voxel_size=0.0), dict(voxel_size=-0.02), dict(voxel_size=nan), dict(voxel_size=1e-50), dict(step=0.0), dict(step=-0.1),
                dict(step=inf), dict(step=1e39), dict(step=1e-50), dict(min_weight=nan), dict(min_weight=inf), dict(range_min=-0.1),
                dict(range_min=2.0, range_max=1.0), dict(range_max=inf), dict(sensor_in_robot=np.full((4, 4), nan))):
        with pytest.raises(ValueError):
            ops.tsdf_raycast_params(cam, **bad)
    with pytest.raises(ValueError):
        ops.tsdf_raycast_params(dict(cam, fx=nan))

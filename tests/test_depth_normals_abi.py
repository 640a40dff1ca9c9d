"""The second public header, include/proslam_hip_normals.h, as the C compiler lays it out against its binding
srrg2_proslam_amd/_lib_normals.py and the built library: what tests/test_abi_layout.py does for the pinned main header, with the same
helpers (tests/abi_probe.py).  Also the params helper, the null-context refusal and what the header says it leaves out.  No GPU
needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import abi_probe
import test_abi_layout as layout
from srrg2_proslam_amd import _lib, _lib_normals

HEADER = os.path.join(abi_probe.ROOT, "include", "proslam_hip_normals.h")
MIRRORS = [m for m in vars(_lib_normals).values() if isinstance(m, type) and issubclass(m, C.Structure) and m is not C.Structure]


def header_text():
    return open(HEADER).read()


@pytest.fixture(scope="module")
def probe():
    """{"structs": {name: [size, [[field, offset, size], ...]]}, "prototypes": {...}, "main": the main header's constants as this
    header sees them} from a C program that includes the second header alone"""
    text = header_text()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "proslam_hip_normals.h"', "int main(void) {"]
    for struct, fields in abi_probe._declared(text):
        lines.append('  printf("S %s %%lu\\n", (unsigned long) sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('  printf("F %s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s*) 0)->%s));'
                         % (f, struct, f, struct, f))
    for c in ("PRS_ABI_VERSION", "PRS_DEPTH_U16", "PRS_DEPTH_F32", "PRS_OK", "PRS_ERR_NULL", "PRS_ERR_RANGE", "PRS_ERR_UNSUPPORTED"):
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
    return _lib_normals.load()


def test_the_header_adds_to_the_main_header_and_does_not_restate_it(probe):
    text = header_text()
    assert '#include "proslam_hip.h"' in text and "joins it" in text.split("#ifndef")[0]
    assert abi_probe._constant_names(text) == []                       # no constant of its own: the main header's are used
    assert probe["main"] == dict(PRS_ABI_VERSION=104, PRS_DEPTH_U16=0, PRS_DEPTH_F32=1, PRS_OK=0, PRS_ERR_NULL=-1, PRS_ERR_RANGE=-4,
                                 PRS_ERR_UNSUPPORTED=-5)
    assert list(probe["structs"]) == ["prs_depth_normals_params", "prs_depth_normals_batch"]
    assert list(probe["prototypes"]) == ["prs_depth_normals_batch_run", "prs_depth_normals_struct_sizes"]
    main = abi_probe.snapshot()
    assert not set(probe["structs"]) & set(main["structs"]) and not set(probe["prototypes"]) & set(main["prototypes"])
    assert probe["structs"]["prs_depth_normals_params"][0] == 128 and probe["structs"]["prs_depth_normals_batch"][0] == 160
    for name in probe["structs"]:                                       # both end in reserved words
        assert probe["structs"][name][1][-1][0] == "reserved", name


def test_mirrors_have_the_header_layout(probe):
    assert sorted(_lib.c_name(m) for m in MIRRORS) == sorted(probe["structs"])
    for mirror in MIRRORS:
        size, fields = probe["structs"][_lib.c_name(mirror)]
        mine = [[layout.c_field(n), getattr(mirror, n).offset, getattr(mirror, n).size] for n, *_ in mirror._fields_]
        assert C.sizeof(mirror) == size and mine == fields, mirror.__name__


def test_the_main_binding_is_left_alone():
    assert not set(_lib_normals.SYMBOLS) & set(_lib.SYMBOLS)
    assert not [m for m in vars(_lib).values() if isinstance(m, type) and issubclass(m, C.Structure) and m.__module__.endswith("_lib_normals")]
    assert _lib.ABI_VERSION == 104


def test_bindings_match_the_prototypes(probe):
    assert sorted(_lib_normals.SYMBOLS) == sorted(probe["prototypes"])
    wrong = []
    for name, (restype, argtypes) in _lib_normals.SYMBOLS.items():
        ret, params = probe["prototypes"][name]
        assert len(argtypes) == len(params), name
        for where, c_type, bound in [("returns", ret, restype)] + [("argument %d" % i, p, a) for i, (p, a) in enumerate(zip(params, argtypes))]:
            why = layout.bound_as(c_type, bound)
            if why:
                wrong.append("%s %s: %s" % (name, where, why))
    assert not wrong, "\n".join(wrong)


def test_library_exports_both_symbols_and_reports_the_compiled_sizes(probe, built):
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in probe["prototypes"])
    assert built.prs_version() == 104
    table = dict(_lib_normals.STRUCT_SIZES)
    assert sorted(table) == sorted(n for n in probe["prototypes"] if n.endswith("_struct_sizes"))
    for query, mirrors in table.items():
        count = int(re.search(r"\b%s\(uint64_t\* sizes(\d+)\)" % query, header_text()).group(1))
        assert len(mirrors) == count
        sizes = (C.c_uint64 * count)()
        getattr(built, query)(sizes)
        assert list(sizes) == [probe["structs"][_lib.c_name(m)][0] for m in mirrors]


def test_header_says_what_the_stage_leaves_out():
    text = header_text()
    section = text[text.index(" * Depth normals:"):text.index("} prs_depth_normals_params;")]
    for left_out in ("PCA / plane-fit normals", "curvature", "a bilateral depth pre-filter", "host-pointer variant", "C++ adapter in plugin/"):
        assert left_out in section, left_out


def test_null_context_is_refused(built):
    p, o = _lib_normals.DepthNormalsParams(), _lib_normals.DepthNormalsBatch()
    assert built.prs_depth_normals_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL


def test_params_helper_and_batch_class(built):
    from srrg2_proslam_amd import configs, ops
    assert callable(ops.DepthNormalsBatch) and ops.DepthNormalsBatch.OPTIONAL == ("n_normal",)
    cam = dict(fx=481.2, fy=-480.0, cx=319.5, cy=239.5)
    p = ops.depth_normals_params(cam)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert (p.radius, p.smooth, p.max_rel_diff) == (2, 1, f32(0.05))
    assert (p.range_min, p.range_max, p.depth_type, p.depth_scaling_factor_to_meters) == (f32(0.1), 10.0, ops.DEPTH_U16, 1.0)
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(481.2), -480.0, 319.5, 239.5)
    assert list(p.sensor_in_robot) == list(np.eye(4).reshape(16)) and list(p.reserved) == [0] * 5
    assert configs.DEPTH_NORMALS == dict(radius=2, smooth=1, max_rel_diff=0.05, range_min=0.1, range_max=10.0)
    assert bytes(ops.depth_normals_params(cam, **configs.DEPTH_NORMALS)) == bytes(p)
    S = np.arange(16, dtype=np.float32).reshape(4, 4)
    q = ops.depth_normals_params(cam, 8, 3, 0.0, 0.0, 0.0, "f32", 1e-3, S)
    assert (q.radius, q.smooth, q.max_rel_diff, q.range_min, q.range_max) == (8, 3, 0.0, 0.0, 0.0)
    assert (q.depth_type, q.depth_scaling_factor_to_meters, list(q.sensor_in_robot)) == (ops.DEPTH_F32, f32(1e-3), list(range(16)))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0), dict(radius=9), dict(radius=1.5), dict(smooth=-1), dict(smooth=4), dict(max_rel_diff=-1e-9),
                dict(max_rel_diff=nan), dict(max_rel_diff=inf), dict(max_rel_diff=1e39), dict(depth_type="u8"), dict(depth_type=2),
                dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(range_min=-0.1), dict(range_min=2.0, range_max=1.0),
                dict(range_max=inf), dict(sensor_in_robot=np.full((4, 4), nan))):
        with pytest.raises(ValueError):
            ops.depth_normals_params(cam, **bad)
    with pytest.raises(ValueError):
        ops.depth_normals_params(dict(cam, fx=nan))


def test_write_ply_with_normals(tmp_path):
    from srrg2_proslam_amd import formats
    xyz = np.arange(12, dtype=np.float32).reshape(3, 4)
    normals = -np.arange(12, dtype=np.float32).reshape(3, 4)
    desc = np.arange(96, dtype=np.uint8).reshape(3, 32)
    plain, again, with_n, with_all = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply", "d.ply"))
    formats.write_ply(plain, xyz)
    formats.write_ply(again, xyz, normals=None)
    assert open(plain, "rb").read() == open(again, "rb").read()      # without normals: byte for byte what it was
    assert open(plain, "rb").read() == (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                                        b"property float z\nend_header\n" + xyz[:, :3].tobytes())
    formats.write_ply(with_n, xyz, normals=normals)
    head, body = open(with_n, "rb").read().split(b"end_header\n")
    assert head.decode().split("\n")[3:-1] == ["property float %s" % n for n in ("x", "y", "z", "nx", "ny", "nz")]
    assert body == np.concatenate([xyz[:, :3], normals[:, :3]], axis=1).tobytes()
    formats.write_ply(with_all, xyz[:, :3], desc, normals[:, :3])
    head, body = open(with_all, "rb").read().split(b"end_header\n")
    assert len(head.decode().split("\n")) == 3 + 6 + 32 + 1 and len(body) == 3 * (24 + 32)
    assert np.frombuffer(body, np.uint8).reshape(3, 56)[:, 24:].tobytes() == desc.tobytes()
    for bad in (normals[:2], normals[:, :2], normals.reshape(-1)):
        with pytest.raises(ValueError):
            formats.write_ply(with_n, xyz, normals=bad)

"""The sixth public header, include/proslam_hip_tsdf_mesh.h, as the C compiler lays it out against its binding
srrg2_proslam_amd/_lib_tsdf_mesh.py and the built library: what tests/test_tsdf_raycast_abi.py does for the fourth header, with the
same helpers (tests/abi_probe.py).  Also the null-context refusal, the workspace query, what the header says it leaves out, and
formats.write_ply with faces.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import abi_probe
import test_abi_layout as layout
from srrg2_proslam_amd import _lib, _lib_dense_align, _lib_normals, _lib_tsdf, _lib_tsdf_mesh, _lib_tsdf_raycast, formats

HEADER = os.path.join(abi_probe.ROOT, "include", "proslam_hip_tsdf_mesh.h")
MIRRORS = [m for m in vars(_lib_tsdf_mesh).values() if isinstance(m, type) and issubclass(m, C.Structure) and m is not C.Structure]
STRUCTS = ["prs_tsdf_mesh_batch"]
ENTRIES = ["prs_tsdf_mesh_batch_run", "prs_tsdf_mesh_workspace_bytes", "prs_tsdf_mesh_struct_sizes"]


def header_text():
    return open(HEADER).read()


@pytest.fixture(scope="module")
def probe():
    """{"structs": {name: [size, [[field, offset, size], ...]]}, "prototypes": {...}, "main": the main header's constants and the
    third header's params as this header sees them} from a C program that includes the sixth header alone"""
    text = header_text()
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "proslam_hip_tsdf_mesh.h"', "int main(void) {"]
    for struct, fields in abi_probe._declared(text):
        lines.append('  printf("S %s %%lu\\n", (unsigned long) sizeof(%s));' % (struct, struct))
        for f in fields:
            lines.append('  printf("F %s %%lu %%lu\\n", (unsigned long) offsetof(%s, %s), (unsigned long) sizeof(((%s*) 0)->%s));'
                         % (f, struct, f, struct, f))
    for c in ("PRS_ABI_VERSION", "PRS_OK", "PRS_ERR_NULL", "PRS_ERR_CAPACITY", "PRS_ERR_RANGE", "PRS_ERR_UNSUPPORTED"):
        lines.append('  printf("C %s %%lld\\n", (long long) (%s));' % (c, c))
    lines.append('  printf("C sizeof_prs_tsdf_params %lld\\n", (long long) sizeof(prs_tsdf_params));')
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
    return _lib_tsdf_mesh.load()


def test_the_header_adds_to_the_main_header_and_does_not_restate_it(probe):
    text = header_text()
    assert '#include "proslam_hip_tsdf.h"' in text and "joins it" in text.split("#ifndef")[0]
    assert "at the next layout bump" in " ".join(text.split("#ifndef")[0].replace("\n *", " ").split())
    assert abi_probe._constant_names(text) == []                       # no constant of its own: the main header's are used
    assert probe["main"] == dict(PRS_ABI_VERSION=104, PRS_OK=0, PRS_ERR_NULL=-1, PRS_ERR_CAPACITY=-2, PRS_ERR_RANGE=-4,
                                 PRS_ERR_UNSUPPORTED=-5, sizeof_prs_tsdf_params=C.sizeof(_lib_tsdf.TsdfParams))
    assert list(probe["structs"]) == STRUCTS and list(probe["prototypes"]) == ENTRIES
    main = abi_probe.snapshot()
    assert not set(probe["structs"]) & set(main["structs"]) and not set(probe["prototypes"]) & set(main["prototypes"])
    assert [probe["structs"][s][0] for s in STRUCTS] == [152]
    for name in probe["structs"]:                                       # every one ends in reserved words
        assert probe["structs"][name][1][-1][0] == "reserved", name
    batch = [f[0] for f in probe["structs"]["prs_tsdf_mesh_batch"][1]]
    assert batch == ["batch", "nx", "ny", "nz", "vertex_stride", "quad_stride", "origin", "volume", "vertex", "normal", "quad", "cube",
                     "edge", "n_vertices", "n_vertices_total", "n_quads", "n_quads_total", "status", "workspace", "reserved"]
    # the params are the third header's, whose text this pull request leaves as it is: it still lists marching cubes as left out
    third = open(os.path.join(abi_probe.ROOT, "include", "proslam_hip_tsdf.h")).read()
    assert "a triangle mesh (marching cubes)" in third and "mesh_batch" not in third


def test_mirrors_have_the_header_layout(probe):
    assert sorted(_lib.c_name(m) for m in MIRRORS) == sorted(probe["structs"])
    for mirror in MIRRORS:
        size, fields = probe["structs"][_lib.c_name(mirror)]
        mine = [[layout.c_field(n), getattr(mirror, n).offset, getattr(mirror, n).size] for n, *_ in mirror._fields_]
        assert C.sizeof(mirror) == size and mine == fields, mirror.__name__


def test_the_six_bindings_have_no_symbol_in_common():
    names = [set(m.SYMBOLS) for m in (_lib, _lib_normals, _lib_tsdf, _lib_tsdf_raycast, _lib_dense_align, _lib_tsdf_mesh)]
    for i in range(6):
        for j in range(i + 1, 6):
            assert not names[i] & names[j], (i, j)
    assert _lib.ABI_VERSION == 104


def test_bindings_match_the_prototypes(probe):
    assert sorted(_lib_tsdf_mesh.SYMBOLS) == sorted(probe["prototypes"])
    wrong = []
    for name, (restype, argtypes) in _lib_tsdf_mesh.SYMBOLS.items():
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
    table = dict(_lib_tsdf_mesh.STRUCT_SIZES)
    assert sorted(table) == sorted(n for n in probe["prototypes"] if n.endswith("_struct_sizes"))
    for query, mirrors in table.items():
        count = int(re.search(r"\b%s\(uint64_t\* sizes(\d+)\)" % query, header_text()).group(1))
        assert len(mirrors) == count == 1
        sizes = (C.c_uint64 * count)()
        getattr(built, query)(sizes)
        assert list(sizes) == [probe["structs"][_lib.c_name(m)][0] for m in mirrors]


def test_workspace_query(built):
    q = built.prs_tsdf_mesh_workspace_bytes
    # two rows of chunk counts, each rounded up to 16 bytes, and an int32 a voxel
    assert q(1, 2, 2, 2) == 16 + 16 + 32
    assert q(3, 70, 9, 6) == 2 * 48 + 3 * 3780 * 4           # four chunks a sequence
    assert q(1, 1, 1, 1) == 16 + 16 + 16
    assert q(5, 32, 32, 1) == 2 * 32 + 5 * 1024 * 4          # exactly one chunk
    assert q(5, 32, 32, 2) == 2 * 48 + 5 * 2048 * 4
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (-1, 4, 4, 4), (1, 4, 4, -4)):
        assert q(*bad) == 0, bad
    assert q(1, 1024, 1024, 683) == 0                                  # nx * ny * nz beyond (2^31 - 1) / 3
    assert q(1, 1 << 20, 1 << 20, 1) == 0
    assert q(1, 1024, 1024, 682) == 2 * 698368 * 4 + 1024 * 1024 * 682 * 4
    assert q(1 << 14, 32, 32, 1024) == 0                               # batch * chunks beyond 2^24 - 1: no launch holds it
    assert q((1 << 14) - 1, 32, 32, 1024) > 0


def test_header_says_what_the_stage_leaves_out():
    text = header_text()
    section = " ".join(text[text.index(" * TSDF mesh:"):text.index("} prs_tsdf_mesh_batch;")].replace("\n *", " ").split())
    for left_out in ("marching cubes' one-vertex-per-edge mesh", "resolving non-manifold edges", "QEF / dual contouring", "colour",
                     "mesh simplification", "welding across sequences", "host-pointer variant", "C++ adapter in plugin/"):
        assert left_out in section[section.index("Left out:"):], left_out
    assert "FOUR plain launches" in section and "TWO for the count-only call" in section


def test_null_context_is_refused(built):
    p, o = _lib_tsdf.TsdfParams(), _lib_tsdf_mesh.TsdfMeshBatch()
    assert built.prs_tsdf_mesh_batch_run(None, C.byref(p), C.byref(o)) == -1  # PRS_ERR_NULL
    assert built.prs_tsdf_mesh_batch_run(None, None, None) == -1


def test_ops_has_the_batch(built):
    from srrg2_proslam_amd import ops
    assert callable(ops.TsdfMeshBatch) and ops.TSDF_MESH_OUTPUTS == ("normal", "cube", "edge")
    for name in ("descriptor", "run", "count", "mesh_of"):
        assert callable(getattr(ops.TsdfMeshBatch, name)), name


# ---- formats.write_ply(faces=...) ----
def read_ply(path):
    """(header lines, vertex bytes, face records as lists) of a file write_ply wrote, parsed by hand"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    n = int([h for h in header if h.startswith("element vertex")][0].split()[2])
    first_face = [i for i, h in enumerate(header) if h.startswith("element face")]
    properties = header[3:first_face[0] if first_face else -1]
    size = sum(4 if p.split()[1] == "float" else 1 for p in properties)
    body = raw[end:]
    faces, at = [], n * size
    if first_face:
        for _ in range(int(header[first_face[0]].split()[2])):
            count = body[at]
            faces.append(np.frombuffer(body[at + 1:at + 1 + 4 * count], "<i4").tolist())
            at += 1 + 4 * count
    assert at == len(body)
    return header, body[:n * size], faces


@pytest.mark.parametrize("width", [3, 4])
def test_write_ply_with_faces(tmp_path, width):
    rng = np.random.default_rng(3)
    xyz, normals = rng.normal(size=(7, 4)).astype(np.float32), rng.normal(size=(7, 4)).astype(np.float32)
    faces = rng.integers(0, 7, (5, width)).astype(np.int32)
    faces[0, 0], faces[1, 1] = 0, 6                                     # both ends of the range
    plain, with_faces = str(tmp_path / "plain.ply"), str(tmp_path / "faces.ply")
    formats.write_ply(plain, xyz, normals=normals)
    formats.write_ply(with_faces, xyz, normals=normals, faces=faces)
    header, vertices, got = read_ply(with_faces)
    assert header == ["ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y",
                      "property float z", "property float nx", "property float ny", "property float nz", "element face 5",
                      "property list uchar int vertex_indices", "end_header"]
    assert got == faces.tolist()
    plain_header, plain_vertices, none = read_ply(plain)
    assert none == [] and plain_vertices == vertices and plain_header == header[:9] + ["end_header"]
    assert vertices == np.concatenate([xyz[:, :3], normals[:, :3]], axis=1).astype("<f4").tobytes()
    # other integer types are taken as they are, and an empty list of faces is a face element of 0
    formats.write_ply(str(tmp_path / "i64.ply"), xyz, normals=normals, faces=faces.astype(np.int64))
    assert open(str(tmp_path / "i64.ply"), "rb").read() == open(with_faces, "rb").read()
    formats.write_ply(str(tmp_path / "none.ply"), xyz, faces=np.zeros((0, width), np.int32))
    assert read_ply(str(tmp_path / "none.ply"))[0][-3:] == ["element face 0", "property list uchar int vertex_indices", "end_header"]


def test_write_ply_without_faces_is_what_it_was(tmp_path):
    xyz = np.arange(12, dtype=np.float32).reshape(4, 3)
    desc = np.arange(128, dtype=np.uint8).reshape(4, 32)
    path = str(tmp_path / "cloud.ply")
    formats.write_ply(path, xyz, desc)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n" + \
        "".join("property uchar d%d\n" % i for i in range(32)) + "end_header\n"
    rows = b"".join(xyz[i].astype("<f4").tobytes() + desc[i].tobytes() for i in range(4))
    assert open(path, "rb").read() == header.encode("ascii") + rows
    formats.write_ply(path, xyz, desc, None, None)
    assert open(path, "rb").read() == header.encode("ascii") + rows


def test_write_ply_refuses_faces_it_cannot_write(tmp_path):
    xyz = np.zeros((4, 3), np.float32)
    path = str(tmp_path / "bad.ply")
    for bad in (np.array([[0, 1, 4]]), np.array([[0, -1, 2]]), np.array([[0, 1, 2, 4]]), np.array([[0, 1]]), np.array([0, 1, 2]),
                np.array([[0.0, 1.0, 2.0]]), np.array([[0, 1, 2, 3, 0]])):
        with pytest.raises(ValueError):
            formats.write_ply(path, xyz, faces=bad)
    assert not os.path.exists(path)
    with pytest.raises(ValueError):
        formats.write_ply(path, np.zeros((0, 3), np.float32), faces=np.array([[0, 0, 0]]))

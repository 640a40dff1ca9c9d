"""The RGB-D preprocessor on the device (srrg2_proslam_amd/csrc/rgbd.hip) against the numpy checker (tests/rgbd_ref.py): keypoints,
depth bits, descriptors, intensities, n_fixed and status, on the ICL frames behind both extractors and on hand-made keypoints and
depth images at the rounding, depth-value, pitch, count and status edges; one graph capture; the C++ adapter; the ICL tracker fed
by the device stage; and a device-resident RGB-D chain extract -> depth -> clip -> align -> compose -> merge against the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_pins as rp
import ref_tracker as rt
import rgbd_ref as rr
from helpers import aligner_params as oracle_aligner_params, corr_equal, pcf_params_from_cfg
from oracle import binding_features as of
from oracle import binding_mapping as om
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn
from test_ref_pins_gpu import HipBackend
from test_ref_tracker import OracleStages
from test_ref_tracker_gpu import HipStages
from tests.test_mapping_gpu import _assert_map_equal, _gpu_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
F_MM = np.float32(1e-3)
ICL = (0, 1, 50)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _icl_mm(k):
    return rp.load("ref_icl")["depth_mm"][{0: 0, 1: 1, 50: 2}[k]]


def _run(ctx, depth, kps, scale, stride=None, extra_pitch_bytes=0, n_features=None, extract_status=None, with_intensity=True, seed=0):
    """depth: numpy [B, rows, cols] uint16 / float32; kps: list of [n_b, 2] float32.  Uploads random descriptors and intensities,
    runs prs_depth_measurements_batch once and returns (inputs, outputs) as numpy"""
    B, rows, cols = depth.shape
    elem = depth.dtype.itemsize
    assert extra_pitch_bytes % elem == 0
    pcols = cols + extra_pitch_bytes // elem
    dbuf = np.zeros((B, rows, pcols), depth.dtype)
    dbuf[:, :, :cols] = depth
    dev_depth = _t(dbuf)[:, :, :cols]
    assert dev_depth.stride(1) * elem == pcols * elem
    n = [len(k) for k in kps] if n_features is None else list(n_features)
    stride = stride or max(max(len(k) for k in kps), 1)
    rng = np.random.default_rng(seed)
    kp = np.zeros((B, stride, 2), np.float32)
    for b, k in enumerate(kps):
        kp[b, : min(len(k), stride)] = np.asarray(k, np.float32)[:stride]
    desc = rng.integers(0, 256, (B, stride, 32), dtype=np.uint8)
    inten = rng.uniform(0, 255, (B, stride)).astype(np.float32)
    fixed = torch.full((B, stride, 4), -7.0, dtype=torch.float32, device=DEV)
    fdesc = torch.zeros((B, stride, 32), dtype=torch.uint8, device=DEV)
    fint = torch.zeros((B, stride), dtype=torch.float32, device=DEV) if with_intensity else None
    n_fixed = torch.full((B,), -99, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -99, dtype=torch.int32, device=DEV)
    es = _t(np.asarray(extract_status, np.int32)) if extract_status is not None else None
    dt = "u16" if depth.dtype == np.uint16 else "f32"
    ops.depth_measurements_batch(ctx, ops.depth_params(dt, scale), dev_depth, _t(kp), _t(desc), _t(np.asarray(n, np.int32)), fixed, fdesc,
                                 n_fixed, status, _t(inten) if with_intensity else None, fint, es)
    torch.cuda.synchronize()
    out = dict(fixed=fixed.cpu().numpy(), desc=fdesc.cpu().numpy(), inten=fint.cpu().numpy() if with_intensity else None,
               n_fixed=n_fixed.cpu().numpy(), status=status.cpu().numpy())
    return dict(depth=depth, kp=kp, desc=desc, inten=inten, n=n, stride=stride, es=extract_status, scale=scale), out


def _same(inp, out, b, with_intensity=True):
    """frame b of a run equals the checker; returns the checker's status"""
    es = 0 if inp["es"] is None else int(inp["es"][b])
    n = inp["n"][b]
    uvd, desc, inten, status = rr.measurements(inp["depth"][b], inp["kp"][b][: min(n, inp["stride"])], inp["desc"][b][: min(n, inp["stride"])],
                                               inp["scale"], inp["inten"][b][: min(n, inp["stride"])], n_features=n, stride=inp["stride"],
                                               extract_status=es)
    assert int(out["status"][b]) == status, (b, int(out["status"][b]), status)
    if status < 0:
        assert int(out["n_fixed"][b]) == 0, b
        return status
    k = len(uvd)
    assert int(out["n_fixed"][b]) == k, (b, int(out["n_fixed"][b]), k)
    assert np.array_equal(_bits(out["fixed"][b, :k, :3]), _bits(uvd)), b
    assert np.all(_bits(out["fixed"][b, :k, 3]) == 0), b
    assert np.array_equal(out["desc"][b, :k], desc), b
    if with_intensity:
        assert np.array_equal(_bits(out["inten"][b, :k]), _bits(inten)), b
    return status


# ---- the ICL frames behind the two extractors ----

@pytest.fixture(scope="module")
def icl_frames(hip_ctx):
    hip_ctx.use_torch_stream()
    cfg = configs.get("icl")
    fr = ops.RGBDFrames(0, 3, 480, 640, 2048)
    for b, k in enumerate(ICL):
        fr.upload(b, rp.icl_gray(k), _icl_mm(k))
    ep, dp = ops.rgbd_params(cfg)
    return fr, ep, dp


def _extractor_outputs(fr, b):
    n = int(fr.n_features[b].item())
    return fr.keypoints[b, :n].cpu().numpy(), fr.descriptors[b, :n].cpu().numpy(), fr.intensity[b, :n].cpu().numpy()


@pytest.mark.parametrize("depth_type", ["u16", "f32"])
def test_icl_frames_through_the_binned_extractor(hip_ctx, icl_frames, depth_type):
    fr, ep, dp = icl_frames
    if depth_type == "f32":  # the fixture's metre image (fixtures.hpp:737-740) with scale 1: the same bits
        frf = ops.RGBDFrames(0, 3, 480, 640, 2048, depth_type="f32")
        for b, k in enumerate(ICL):
            frf.upload(b, rp.icl_gray(k), rp.icl_depth_m(k))
        fr, dp = frf, ops.depth_params("f32", 1.0)
    fr.run(hip_ctx, ep, dp)
    torch.cuda.synchronize()
    B = HipBackend(hip_ctx)
    for b, k in enumerate(ICL):
        uv, desc, inten = _extractor_outputs(fr, b)
        depth = _icl_mm(k) if depth_type == "u16" else rp.icl_depth_m(k)
        want_uvd, want_desc, want_int, want_status = rr.measurements(depth, uv, desc, dp.depth_scaling_factor_to_meters, inten)
        uvd, gdesc, gint, status = fr.fixed_of(b)
        assert status == want_status and len(uvd) > 200
        assert np.array_equal(_bits(uvd), _bits(want_uvd)) and np.array_equal(gdesc, want_desc) and np.array_equal(_bits(gint), _bits(want_int))
        # the ICL fixture's own lookup on the HIP extractor's keypoints (tests/ref_pins.py::icl_measurements)
        ref = rp.icl_measurements(B, k)
        assert np.array_equal(_bits(uvd[:, :2]), _bits(ref["uv"])) and np.array_equal(_bits(uvd[:, 2]), _bits(ref["depth"]))
        # the host entry point gives the same
        h_uvd, h_int, h_desc, h_status = ops.depth_measurements(hip_ctx, dp, depth, uv, desc, inten)
        assert h_status == status and np.array_equal(_bits(h_uvd), _bits(uvd)) and np.array_equal(h_desc, gdesc)
        assert np.array_equal(_bits(h_int), _bits(gint))


def test_icl_frames_through_the_selective_extractor(hip_ctx, icl_frames):
    fr, _, dp = icl_frames
    sp = ops.selective_extractor_params("GFTT", target_number_of_keypoints=800)
    ops.extract_features_selective_batch(hip_ctx, sp, fr.images, fr.keypoints, fr.descriptors, fr.n_features, fr.status, fr.intensity)
    fr.measure(hip_ctx, dp)
    torch.cuda.synchronize()
    for b, k in enumerate(ICL):
        uv, desc, inten = _extractor_outputs(fr, b)
        assert len(uv) > 50
        want_uvd, want_desc, want_int, want_status = rr.measurements(_icl_mm(k), uv, desc, F_MM, inten)
        uvd, gdesc, gint, status = fr.fixed_of(b)
        assert status == want_status
        assert np.array_equal(_bits(uvd), _bits(want_uvd)) and np.array_equal(gdesc, want_desc) and np.array_equal(_bits(gint), _bits(want_int))


# ---- hand-made keypoints and depth images ----

@pytest.mark.parametrize("cols", [63, 64])
@pytest.mark.parametrize("depth_type", [np.uint16, np.float32])
def test_half_pixel_keypoints(hip_ctx, cols, depth_type):
    rows, B = 47, 4
    rng = np.random.default_rng(cols)
    depth = rng.integers(0, 4, (B, rows, cols)).astype(depth_type)  # a quarter of the pixels without depth
    kps = []
    for b in range(B - 1):
        u = rng.integers(-1, cols - 1, 700) + np.float32(0.5)  # -0.5 .. cols - 1.5
        v = rng.integers(-1, rows - 1, 700) + np.float32(0.5)
        u[:4] = [-0.5, cols - 1.5, cols - 0.5 if cols % 2 else cols - 1.5, 0.5]
        v[:4] = [-0.5, rows - 1.5, 0.5, rows - 0.5 if rows % 2 else rows - 1.5]  # rows 47: 46.5 rounds to 46, inside
        kps.append(np.stack([u, v], axis=1).astype(np.float32))
    # last frame: u = cols - 0.5, which rounds outside for even cols (63.5 -> 64) and inside for odd cols (62.5 -> 62)
    kps.append(np.array([[1.0, 1.0], [cols - 0.5, 3.0]], np.float32))
    inp, out = _run(hip_ctx, depth, kps, 0.25)
    for b in range(B - 1):
        assert _same(inp, out, b) >= 0
    assert (_same(inp, out, B - 1) == rr.ERR_RANGE) == (cols % 2 == 0)


def test_depth_value_edges(hip_ctx):
    tiny = np.float32(np.finfo(np.float32).smallest_subnormal)
    vals = np.array([0.0, -0.0, -3.0, np.nan, np.inf, tiny, 1.5, 7e-3, -np.inf, 1e30], np.float32)
    depth = np.tile(vals, (2, 5, 3))[:, :, :30]
    kp = np.stack(np.meshgrid(np.arange(30, dtype=np.float32), np.arange(5, dtype=np.float32)), axis=-1).reshape(-1, 2)
    for scale in (F_MM, 1.0, 1e-30, -2.0, 0.0):
        inp, out = _run(hip_ctx, depth, [kp, kp[::-1]], scale)
        assert _same(inp, out, 0) == rr.WARN_SPARSE_DEPTH and _same(inp, out, 1) == rr.WARN_SPARSE_DEPTH
    u16 = np.array([[[0, 1, 65535, 2]]], np.uint16)
    inp, out = _run(hip_ctx, u16, [np.array([[0, 0], [1, 0], [2, 0], [3, 0]], np.float32)], F_MM)
    assert _same(inp, out, 0) == 0 and int(out["n_fixed"][0]) == 3
    assert _bits(out["fixed"][0, 1, 2]) == _bits(np.float32(65535) * F_MM)


@pytest.mark.parametrize("extra", [2, 64])
@pytest.mark.parametrize("depth_type", [np.uint16, np.float32])
def test_depth_pitch(hip_ctx, extra, depth_type):
    rows, cols, B = 37, 45, 3
    rng = np.random.default_rng(extra)
    depth = rng.integers(0, 5, (B, rows, cols)).astype(depth_type)
    elem = np.dtype(depth_type).itemsize
    kps = [np.stack([rng.integers(0, cols, 500), rng.integers(0, rows, 500)], axis=1).astype(np.float32) for _ in range(B)]
    kps[1][:2] = [[cols - 1, rows - 1], [cols - 1, 0]]  # the last column: the bytes behind it are padding
    inp, out = _run(hip_ctx, depth, kps, 1.0, extra_pitch_bytes=extra * elem if extra == 2 else extra)
    for b in range(B):
        assert _same(inp, out, b) >= 0


def test_feature_counts(hip_ctx):
    rows, cols = 64, 80
    counts = [0, 1, 63, 64, 65, 255, 256, 257, 4096]
    rng = np.random.default_rng(3)
    depth = rng.integers(0, 3, (len(counts), rows, cols)).astype(np.uint16)
    kps = [np.stack([rng.uniform(-0.5, cols - 0.5, n), rng.uniform(-0.5, rows - 0.5, n)], axis=1).astype(np.float32) for n in counts]
    for k in kps:  # keep them inside after rounding
        k[:, 0] = np.clip(k[:, 0], 0, cols - 1)
        k[:, 1] = np.clip(k[:, 1], 0, rows - 1)
    inp, out = _run(hip_ctx, depth, kps, 1.0, stride=4096)
    for b, n in enumerate(counts):
        st = _same(inp, out, b)
        assert (st == rr.WARN_NO_MATCHES) == (n == 0 or int(out["n_fixed"][b]) == 0)
    # n == stride, without intensity
    inp, out = _run(hip_ctx, depth[:2], [kps[5], kps[6][:255]], 1.0, stride=255, with_intensity=False)
    assert _same(inp, out, 0, with_intensity=False) >= 0 and _same(inp, out, 1, with_intensity=False) >= 0


def test_sparse_depth_threshold(hip_ctx):
    rows, cols, n = 16, 32, 256
    depth = np.ones((3, rows, cols), np.float32)
    kp = np.stack([np.arange(n) % cols, np.arange(n) // cols], axis=1).astype(np.float32)
    for b, holes in enumerate((64, 65, 255)):  # 64 / 256 = 0.25 exactly: no warning; 65: above; 255: one kept
        depth[b].reshape(-1)[np.random.default_rng(b).choice(n, holes, replace=False)] = 0
    inp, out = _run(hip_ctx, depth, [kp] * 3, 1.0)
    assert [_same(inp, out, b) for b in range(3)] == [0, rr.WARN_SPARSE_DEPTH, rr.WARN_SPARSE_DEPTH]
    assert list(out["n_fixed"]) == [192, 191, 1]


def test_per_frame_errors_leave_the_other_frames_exact(hip_ctx):
    rows, cols, B, stride = 30, 40, 7, 300
    rng = np.random.default_rng(11)
    depth = rng.integers(0, 3, (B, rows, cols)).astype(np.uint16)
    kps = [np.stack([rng.integers(0, cols, 280), rng.integers(0, rows, 280)], axis=1).astype(np.float32) for _ in range(B)]
    kps[2][270] = [cols + 0.7, 3.0]  # range error in the second chunk
    kps[4][3] = [2.0, -0.7]           # range error in the first chunk
    n = [280] * B
    n[3] = stride + 1                 # more features than the stride
    es = [0, -2, 0, 0, 0, rr.WARN_NO_MATCHES, 0]  # frame 1: the extractor failed; a warning bit is not an error
    inp, out = _run(hip_ctx, depth, kps, 1.0, stride=stride, n_features=n, extract_status=es)
    assert [_same(inp, out, b) for b in (1, 2, 3, 4)] == [-2, rr.ERR_RANGE, rr.ERR_CAPACITY, rr.ERR_RANGE]
    for b in (0, 5, 6):
        assert _same(inp, out, b) >= 0 and int(out["n_fixed"][b]) > 100


def test_extract_status_may_alias_status(hip_ctx, icl_frames):
    fr, ep, dp = icl_frames
    fr.extract(hip_ctx, ep)
    fr.status[1] = -2  # as if the extractor had failed on frame 1
    fr.measure(hip_ctx, dp)  # extract_status is fr.status
    torch.cuda.synchronize()
    assert [int(fr.status[b]) for b in range(3)][1] == -2 and int(fr.n_fixed[1]) == 0
    assert int(fr.status[0]) >= 0 and int(fr.n_fixed[0]) > 200


def test_call_level_errors(hip_ctx):
    lib = _lib.load()
    depth = torch.ones((1, 8, 8), dtype=torch.uint16, device=DEV)
    kp = torch.zeros((1, 4, 2), dtype=torch.float32, device=DEV)
    desc = torch.zeros((1, 4, 32), dtype=torch.uint8, device=DEV)
    n = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    fixed = torch.zeros((1, 4, 4), dtype=torch.float32, device=DEV)
    fdesc = torch.zeros((1, 4, 32), dtype=torch.uint8, device=DEV)
    nf, st = torch.zeros((1,), dtype=torch.int32, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
    inten = torch.zeros((1, 4), dtype=torch.float32, device=DEV)

    def call(params, **over):
        d = _lib.DepthBatch()
        d.batch, d.rows, d.cols, d.pitch, d.depth, d.stride = 1, 8, 8, 16, depth.data_ptr(), 4
        d.keypoints, d.descriptors, d.n_features = kp.data_ptr(), desc.data_ptr(), n.data_ptr()
        d.fixed, d.fixed_desc, d.n_fixed, d.status = fixed.data_ptr(), fdesc.data_ptr(), nf.data_ptr(), st.data_ptr()
        for k, v in over.items():
            setattr(d, k, v)
        return lib.prs_depth_measurements_batch(hip_ctx._h, C.byref(params), C.byref(d))

    good = ops.depth_params("u16", 1.0)
    assert call(good) == 0
    assert call(ops.depth_params(2, 1.0)) == _lib.ERR_UNSUPPORTED
    for s in (float("nan"), float("inf"), -float("inf")):
        assert call(ops.depth_params("u16", s)) == _lib.ERR_RANGE
    for over in (dict(pitch=15), dict(pitch=14), dict(rows=0), dict(cols=0), dict(stride=0)):
        assert call(good, **over) == _lib.ERR_RANGE, over
    assert call(ops.depth_params("f32", 1.0), pitch=18) == _lib.ERR_RANGE  # a multiple of 2, not of 4
    for name in ("depth", "keypoints", "descriptors", "n_features", "fixed", "fixed_desc", "n_fixed", "status"):
        assert call(good, **{name: None}) == _lib.ERR_NULL, name
    assert call(good, intensity=inten.data_ptr()) == _lib.ERR_NULL  # intensity without fixed_intensity
    assert call(good, fixed_intensity=inten.data_ptr()) == _lib.ERR_NULL
    assert lib.prs_depth_measurements_batch(hip_ctx._h, None, None) == _lib.ERR_NULL
    torch.cuda.synchronize()
    # the host entry point
    d16 = np.ones((8, 8), np.uint16)
    with pytest.raises(ops.ProslamHipError) as e:
        ops.depth_measurements(hip_ctx, ops.depth_params(5, 1.0), d16, [[1, 1]], np.zeros((1, 32), np.uint8))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(ops.ProslamHipError) as e:
        ops.depth_measurements(hip_ctx, ops.depth_params("u16", float("nan")), d16, [[1, 1]], np.zeros((1, 32), np.uint8))
    assert e.value.status == _lib.ERR_RANGE
    with pytest.raises(ops.ProslamHipError) as e:
        ops.depth_measurements(hip_ctx, ops.depth_params("u16", 1.0), d16, [[8.5, 1]], np.zeros((1, 32), np.uint8))
    assert e.value.status == _lib.ERR_RANGE
    uvd, _, _, status = ops.depth_measurements(hip_ctx, ops.depth_params("u16", 1.0), d16, np.zeros((0, 2)), np.zeros((0, 32), np.uint8))
    assert len(uvd) == 0 and status == _lib.WARN_NO_MATCHES


# ---- graph capture ----

def test_graph_capture_replays_extraction_and_depth(icl_frames):
    _, ep, dp = icl_frames
    ctx = ops.Context(0)
    fr = ops.RGBDFrames(0, 3, 480, 640, 2048)
    sets = [[rp.icl_gray(k) for k in ICL], [rp.icl_gray(k)[::-1].copy() for k in ICL]]
    depths = [[_icl_mm(k) for k in ICL], [_icl_mm(k)[:, ::-1].copy() for k in ICL]]
    eager = []
    for imgs, deps in zip(sets, depths):
        for b in range(3):
            fr.upload(b, imgs[b], deps[b])
        ctx.use_torch_stream()
        fr.run(ctx, ep, dp)  # also allocates the extractor's scratch before the capture
        torch.cuda.synchronize()
        eager.append([fr.fixed_of(b) for b in range(3)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fr.run(ctx, ep, dp)
        for imgs, deps, want in zip(sets, depths, eager):
            for b in range(3):
                fr.upload(b, imgs[b], deps[b])
            fr.n_fixed.fill_(-1)
            fr.fixed.fill_(-1.0)
            side.synchronize()
            graph.replay()
            side.synchronize()
            for b in range(3):
                uvd, desc, inten, status = fr.fixed_of(b)
                assert status == want[b][3] and np.array_equal(_bits(uvd), _bits(want[b][0])), b
                assert np.array_equal(desc, want[b][1]) and np.array_equal(_bits(inten), _bits(want[b][2]))
    torch.cuda.synchronize()
    del graph
    ctx.close()


# ---- the C++ adapter ----

def test_cpp_rgbd_adapter(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "test_rgbd_plugin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    gray, mm = rp.icl_gray(0), _icl_mm(0)
    (tmp_path / "gray.raw").write_bytes(np.ascontiguousarray(gray).tobytes())
    (tmp_path / "depth.raw").write_bytes(np.ascontiguousarray(mm, np.uint16).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(tmp_path / "gray.raw"), str(tmp_path / "depth.raw"), str(gray.shape[0]), str(gray.shape[1]),
                        str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.count("[  OK  ]") == 3 and "FAILED" not in out and "0 failure(s)" in out, out
    raw = (tmp_path / "out.bin").read_bytes()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    rec = np.frombuffer(raw[4:], dtype=np.dtype([("uvd", np.float32, 3), ("inten", np.float32), ("desc", np.uint8, 32)]))
    assert len(rec) == n
    uv, inten, desc = of.extract_features(of.extractor_params(5, 1, 500, 3, 3, of.SELECT_LIBSTDCXX), gray, capacity=4096)
    want_uvd, want_desc, want_int, _ = rr.measurements(mm, uv, desc, F_MM, inten)
    assert np.array_equal(_bits(rec["uvd"]), _bits(want_uvd)) and np.array_equal(rec["desc"], want_desc)
    assert np.array_equal(_bits(rec["inten"]), _bits(want_int))


# ---- the ICL tracker scenario fed by the device stage ----

def test_icl_tracker_fed_by_the_device_stage(hip_ctx, icl_frames, oracle):
    fr, ep, dp = icl_frames
    fr.run(hip_ctx, ep, dp)
    torch.cuda.synchronize()
    meas = [fr.fixed_of(b) for b in range(3)]
    assert all(m[3] >= 0 for m in meas)
    cfg, merger = rt.icl_setup()
    t = rt.Tracker(HipStages(hip_ctx), cfg, merger)
    log = [t.process(m[0], m[1]) for m in meas]
    error = rp.t2tnq(np.linalg.inv(np.asarray(t.pose, np.float64)) @ rp.icl_relative(50, 0))
    assert np.all(np.abs(error[:3]) < 0.02) and np.all(np.abs(error[3:]) < 0.01), error
    ref, ref_error = rt.icl_00_01_50(HipStages(hip_ctx), HipBackend(hip_ctx))
    for k, (e, o) in enumerate(zip(log, ref)):
        for key in ("n_measured", "map_size", "merged", "added", "status", "inliers", "n_corr", "n_clipped"):
            assert e.get(key) == o.get(key), (k, key, e.get(key), o.get(key))
        assert np.array_equal(_bits(e["pose"]), _bits(o["pose"])), k
    assert np.array_equal(np.asarray(error), np.asarray(ref_error))


# ---- a device-resident RGB-D chain against the oracle ----

def test_rgbd_images_to_poses_matches_the_oracle_chain(oracle, hip_ctx):
    """extract -> depth -> clip -> align (icl) -> compose -> merge (PRS_MERGER_DEPTH_EKF) with no host copy between stages, the
    counterpart of test_images_to_poses_matches_the_oracle_chain; the scene is the layered one of synthetic.rgbd_image_sequence"""
    cfg, merger = rt.icl_setup()
    B, n_frames, stride, cap = 2, 4, 1024, 3000
    seqs = [syn.rgbd_image_sequence(np.random.default_rng(80 + b), cfg, n_frames) for b in range(B)]
    step = seqs[0][1]
    stages = OracleStages()
    po = stages.new_map(cfg, merger, cap)["params"]
    pg = _gpu_params(po)
    hip_ctx.use_torch_stream()
    ep, dp = ops.rgbd_params(cfg)

    rf = ops.RGBDFrames(0, B, cfg["camera"]["rows"], cfg["camera"]["cols"], stride)
    maps = ops.MapBatch(0, B, cap, 0, n_frames + 1, stride, stride)
    maps.measurement, maps.measurement_desc, maps.n_measured = rf.fixed, rf.fixed_desc, rf.n_fixed
    clip = ops.ClipScenes(0, B, cap)
    clip.scene_xyzw, clip.scene_desc, clip.n_scene, clip.scene_n_opt = maps.coords, maps.desc, maps.n_points, maps.n_opt
    af = ops.AlignFrames(0, B, stride, cap)
    af.fixed, af.fixed_desc, af.n_fixed = rf.fixed, rf.fixed_desc, rf.n_fixed
    af.moving, af.moving_desc, af.n_moving = clip.clipped_xyzw, clip.clipped_desc, clip.n_clipped
    maps.corr, maps.corr_from_aligner, maps.scene_index_map = af.corr, 1, clip.global_indices
    state0 = af.state.clone()
    pose = torch.eye(4, dtype=torch.float32, device=DEV).repeat(B, 1, 1).contiguous()
    eye16 = torch.eye(4, dtype=torch.float32, device=DEV).reshape(1, 16).repeat(B, 1).contiguous()
    zero_corr = torch.zeros((B,), dtype=torch.int32, device=DEV)
    pp, apar = ops.pcf_params(cfg), ops.aligner_params(cfg)
    I4 = np.eye(4, dtype=np.float32)

    omaps = [om.Map(cap, 0) for _ in range(B)]
    oposes = [om.pose_table(n_frames + 1) for _ in range(B)]
    opose = [I4.copy() for _ in range(B)]
    eo = of.extractor_params(5, 1, 500, 3, 3, of.SELECT_LIBSTDCXX)

    for k in range(n_frames):
        for b in range(B):
            rf.upload(b, *seqs[b][0][k])
        # device chain
        rf.run(hip_ctx, ep, dp)
        if k > 0:
            clip.robot_in_local_map.copy_(pose)
            af.state.copy_(state0)
            af.X.copy_(eye16)
            af.n_corr.zero_()
            ops.scene_clip_batch(hip_ctx, pp.projector, I4, clip)
            ops.align_batch(hip_ctx, pp, apar, af)
            ops.pose_compose_batch(hip_ctx, clip.robot_in_local_map, af.X, pose)
            maps.n_corr = af.n_corr
        else:
            maps.n_corr = zero_corr
        maps.measurement_in_world.copy_(pose)
        maps.measurement_in_scene.copy_(pose)
        maps.frame.fill_(k)
        ops.merge_batch(hip_ctx, pg, maps)
        torch.cuda.synchronize()
        # oracle chain: the CPU extractor, the checker, the CPU finder / aligner / merger
        for b in range(B):
            gray, mm = seqs[b][0][k]
            uv, inten, desc = of.extract_features(eo, gray, capacity=4096)
            fixed, fdesc, _, want_status = rr.measurements(mm, uv, desc, F_MM, inten)
            uvd, gdesc, _, status = rf.fixed_of(b)
            assert status == want_status and np.array_equal(_bits(uvd), _bits(fixed)) and np.array_equal(gdesc, fdesc), (k, b, "depth stage")
            assert len(fixed) > 250
            c, imap = np.zeros(0, oracle.CORR_DTYPE), None
            m = omaps[b]
            if k > 0:
                xyzw = m.coords[: m.n_points].copy()
                xyzw[:, 3] = oracle.info_scale_from_nopt(m.n_opt[: m.n_points])
                cx, cd, gi, _ = oracle.scene_clip(pcf_params_from_cfg(oracle, cfg).projector, opose[b], I4, xyzw, m.desc[: m.n_points])
                f = oracle.ProjectiveFinder(pcf_params_from_cfg(oracle, cfg))
                f.set_fixed(fixed, fdesc)
                f.set_moving(cx[:, :3], cd)
                res, rc = oracle.align_frame(f, oracle_aligner_params(oracle, cfg, mean_disparity=0.0), fixed, cx[:, :3], cx[:, 3], I4)
                f.close()
                assert corr_equal(rc, af.corr_of(b)), (k, b, "aligner correspondences")
                assert res.status == 1 and len(rc) > 60
                opose[b] = oracle.se3_mul(opose[b], oracle.se3_inverse(np.array(res.X, np.float32).reshape(4, 4)))
                assert np.array_equal(_bits(opose[b]).ravel(), _bits(pose[b].cpu().numpy()).ravel()), (k, b, "pose")
                c = rc.copy()
                c["fixed_idx"], c["moving_idx"] = rc["moving_idx"], rc["fixed_idx"]
                imap = np.concatenate([gi, np.zeros(cap - len(gi), np.int32)])
            rcode, mres = om.merge(po, opose[b], opose[b], oposes[b], k, m, fixed, fdesc, c, imap)
            assert rcode == 0
            got = maps.result[b].cpu().numpy()
            assert (int(got[0]), int(got[1]), int(got[2])) == (mres.n_merged, mres.n_added, mres.flags), (k, b)
            _assert_map_equal(maps, b, m, oposes[b], k + 1)
            truth = np.array([k * step, 0.0, 0.0], np.float32)
            assert np.linalg.norm(opose[b][:3, 3] - truth) < 0.01, (k, b, opose[b][:3, 3], truth)
    assert all(m.n_points > 400 for m in omaps)

"""The image rectifier on the device against its float32 numpy restatement (tests/rectify_ref.py), byte for byte: dst, n_border, status,
and the pitch padding of dst, which is prefilled with a pattern and must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import rectify_ref as ref
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu

PAD = 0xA5
D0 = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)  # EuRoC cam0
ERR_NULL, ERR_RANGE, ERR_UNSUPPORTED = -1, -4, -5


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def kmat(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def make_map(kind, src_shape, dst_shape=None):
    """the maps of the issue's list, with EuRoC's intrinsics scaled to the image so that small shapes see the same distortion"""
    rows, cols = src_shape
    drows, dcols = src_shape if dst_shape is None else dst_shape
    s, cam = cols / 752.0, configs.EUROC["camera"]
    Ks = kmat(458.654 * s, 457.296 * s, 367.215 * s, 248.375 * rows / 480.0)
    Kd = kmat(cam["fx"] * dcols / 752.0, cam["fy"] * dcols / 752.0, cam["cx"] * dcols / 752.0, cam["cy"] * drows / 480.0)
    Ki = kmat(64.0, 64.0, float(dcols // 2), float(drows // 2))  # a power of two and integers: every step of the map is exact
    if kind == "identity":
        return ops.rectify_map(Ki, [0] * 5, None, Ki)
    if kind == "shift":  # destination (u, v) samples source (u + 3, v - 2)
        return ops.rectify_map(kmat(64.0, 64.0, Ki[0, 2] + 3, Ki[1, 2] - 2), [0] * 5, None, Ki)
    if kind == "euroc":
        return ops.rectify_map(Ks, D0, rot(1, 0.01) @ rot(0, 0.007), Kd)
    if kind == "strong":  # large, bulging footprints
        return ops.rectify_map(Ks, (-0.45, 0.0, 0.0, 0.0, 0.0), rot(1, np.deg2rad(5.0)), Kd)
    if kind == "wide":  # half the focal length: the destination sees past every edge of the source, along curved lines
        return ops.rectify_map(Ks, D0, rot(2, 0.02), kmat(Kd[0, 0] / 2, Kd[1, 1] / 2, Kd[0, 2], Kd[1, 2]))
    if kind == "far":  # an eighth of the focal length: a tile's source footprint is far larger than the staging buffer
        return ops.rectify_map(Ks, D0, rot(2, 0.02), kmat(Kd[0, 0] / 8, Kd[1, 1] / 8, Kd[0, 2], Kd[1, 2]))
    if kind == "outside":
        return ops.rectify_map(kmat(Ks[0, 0], Ks[1, 1], Ks[0, 2] + 1e5, Ks[1, 2]), D0, None, Kd)
    if kind == "rz_sign":  # rz = R[2] x + R[5] y + R[8] crosses 0 inside the image
        return ops.rectify_map(Ks, D0, rot(1, np.deg2rad(85.0)), Kd)
    raise KeyError(kind)


def image(rng, shape, np_dtype=np.uint8, batch=None):
    full = shape if batch is None else (batch,) + tuple(shape)
    if np_dtype == np.float32:
        return rng.uniform(0.3, 12.0, full).astype(np.float32)
    return rng.integers(0, 256 if np_dtype == np.uint8 else 65536, full).astype(np_dtype)


def run_abi(ctx, params, maps, src, dst_shape=None, map_of=None, src_pitch=None, dst_pitch=None, with_border=True):
    """the bare entry point on images [B, rows, cols] with pitches in ELEMENTS (None: dense) -> (rc, dst, padding_ok, n_border, status)"""
    import torch
    B, rows, cols = src.shape
    drows, dcols = (rows, cols) if dst_shape is None else dst_shape
    sp, dp = src_pitch or cols, dst_pitch or dcols
    host = np.zeros((B, rows, sp), dtype=src.dtype)
    host[:, :, :cols] = src
    d_src = torch.from_numpy(host).cuda()
    d_dst = torch.full((B, drows, dp * src.itemsize), PAD, dtype=torch.uint8, device="cuda")
    arr = (_lib.RectifyMap * len(maps))(*[m.struct() if hasattr(m, "struct") else m for m in maps])
    d_maps = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).cuda()
    d_map_of = None if map_of is None else torch.tensor(list(map_of), dtype=torch.int32, device="cuda")
    n_border = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    d = _lib.RectifyBatch()
    d.batch, d.src_rows, d.src_cols, d.src_pitch, d.src = B, rows, cols, sp * src.itemsize, d_src.data_ptr()
    d.dst_rows, d.dst_cols, d.dst_pitch, d.dst = drows, dcols, dp * src.itemsize, d_dst.data_ptr()
    d.n_maps, d.maps = len(maps), d_maps.data_ptr()
    d.map_of = None if d_map_of is None else d_map_of.data_ptr()
    d.n_border = n_border.data_ptr() if with_border else None
    d.status = status.data_ptr()
    rc = _lib.load().prs_rectify_batch_run(ctx._h, C.byref(params), C.byref(d))
    torch.cuda.synchronize()
    raw = d_dst.cpu().numpy()
    out = np.ascontiguousarray(raw[:, :, :dcols * src.itemsize]).view(src.dtype).reshape(B, drows, dcols)
    padding_ok = bool(np.all(raw[:, :, dcols * src.itemsize:] == PAD))
    return rc, out, padding_ok, n_border.cpu().numpy(), status.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(ctx, params, maps, src, interpolation="bilinear", border=0, dst_shape=None, map_of=None, **pitches):
    rc, got, padding_ok, nb, st = run_abi(ctx, params, maps, src, dst_shape, map_of, **pitches)
    assert rc == 0
    want, wnb, wst = ref.rectify_batch(src, maps, map_of, dst_shape, interpolation, border)
    assert padding_ok, "bytes between dst_cols and dst_pitch were written"
    diff = np.count_nonzero(got.view(np.uint8) != want.view(np.uint8)) if got.shape == want.shape else -1
    assert same_bits(got, want), "%d bytes differ from the float32 restatement" % diff
    assert np.array_equal(nb, wnb) and np.array_equal(st, wst)
    return got, nb, st


# ---- 1. shapes, 2. maps ----
SHAPES = [dict(src=(1, 1)), dict(src=(5, 7)), dict(src=(17, 63)), dict(src=(33, 65), src_pitch=80, dst_pitch=72), dict(src=(480, 752)),
          dict(src=(33, 65), dst=(40, 50))]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%d%s" % (c["src"] + ("_to_%dx%d" % c["dst"] if "dst" in c else "",)))
@pytest.mark.parametrize("kind", ["euroc", "strong"])
def test_shapes(hip_ctx, case, kind):
    rng = np.random.default_rng(sum(case["src"]))
    src = image(rng, case["src"], batch=2)
    m = make_map(kind, case["src"], case.get("dst"))
    check(hip_ctx, ops.rectify_params(border=9), [m], src, border=9, dst_shape=case.get("dst"),
          src_pitch=case.get("src_pitch"), dst_pitch=case.get("dst_pitch"))


@pytest.mark.parametrize("shape", [(33, 65), (480, 752)], ids=["33x65", "480x752"])
def test_maps(hip_ctx, shape):
    rng = np.random.default_rng(3)
    src = image(rng, shape, batch=1)
    P = ops.rectify_params(border=7)
    got, nb, _ = check(hip_ctx, P, [make_map("identity", shape)], src, border=7)
    assert np.array_equal(got, src) and nb[0] == 0
    got, nb, _ = check(hip_ctx, P, [make_map("shift", shape)], src, border=7)
    assert np.array_equal(got[0, 2:, :-3], src[0, :-2, 3:])  # the shifted image ...
    assert np.all(got[0, :2] == 7) and np.all(got[0, :, -3:] == 7)  # ... in a frame of border: vs = -2, -1 and us = cols .. cols + 2
    assert nb[0] == 2 * shape[1] + 3 * (shape[0] - 2)
    for kind in ("euroc", "strong"):
        check(hip_ctx, P, [make_map(kind, shape)], src, border=7)
    for kind in ("wide", "far"):
        _, nb, _ = check(hip_ctx, P, [make_map(kind, shape)], src, border=7)
        assert 0 < nb[0] < shape[0] * shape[1]
    got, nb, st = check(hip_ctx, P, [make_map("outside", shape)], src, border=7)
    assert np.all(got == 7) and nb[0] == shape[0] * shape[1] and st[0] == 0
    got, nb, _ = check(hip_ctx, P, [make_map("rz_sign", shape)], src, border=7)
    _, _, inside = ref.source_positions(make_map("rz_sign", shape), shape, shape)
    assert 0 < nb[0] < shape[0] * shape[1] and inside.any() and not inside.all()


@pytest.mark.parametrize("kind", ["euroc", "strong", "wide"])
def test_taps_from_global_memory(hip_ctx, monkeypatch, kind):
    """tap fetch (a) on the shape that otherwise stages every footprint (b) (PRS_RECTIFY_VARIANT is read per launch)"""
    monkeypatch.setenv("PRS_RECTIFY_VARIANT", "0")
    shape = (480, 752)
    src = image(np.random.default_rng(4), shape, batch=3)
    check(hip_ctx, ops.rectify_params(border=250), [make_map(kind, shape)], src, border=250)


# ---- 3. batches: the held map's switch, an invalid entry, chunks of several images with a short last one ----
def test_batch_map_switch_and_invalid_entry(hip_ctx):
    shape = (33, 65)
    src = image(np.random.default_rng(5), shape, batch=5)
    maps = [make_map("euroc", shape), make_map("strong", shape)]
    P = ops.rectify_params(border=3)
    a, _, st = check(hip_ctx, P, maps, src, border=3, map_of=[1, 0, 1, 1, 0])
    assert not st.any()
    b, _, _ = check(hip_ctx, P, maps, src, border=3, map_of=None)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]) and not np.array_equal(a[0], b[0])
    c, nb, st = check(hip_ctx, P, maps, src, border=3, map_of=[1, 0, 7, 1, 0])
    assert list(st) == [0, 0, ERR_RANGE, 0, 0] and np.all(c[2] == 3) and nb[2] == shape[0] * shape[1]
    assert np.array_equal(np.delete(c, 2, axis=0), np.delete(a, 2, axis=0))
    check(hip_ctx, P, maps, src, border=3, map_of=[-1, 0, 1, 2, 0])
    # a map with a field that is not finite, a zero focal length or an unknown model is refused per image as well
    bad = []
    for field, value in (("k2", float("inf")), ("dst_fy", 0.0), ("model", 1)):
        s = maps[0].struct()
        setattr(s, field, value)
        bad.append(s)
    rc, got, padding_ok, nb, st = run_abi(hip_ctx, P, [maps[0]] + bad, src[:4], map_of=[1, 2, 0, 3])
    assert rc == 0 and padding_ok and list(st) == [ERR_RANGE, ERR_RANGE, 0, ERR_RANGE]
    assert np.all(got[[0, 1, 3]] == 3) and list(nb[[0, 1, 3]]) == [shape[0] * shape[1]] * 3 \
        and np.array_equal(got[2], ref.rectify(src[2], maps[0], border=3)[0])


@pytest.mark.parametrize("chunk", ["16", "3", None], ids=["chunk16", "chunk3", "auto"])
def test_batch_of_40_in_chunks(hip_ctx, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("PRS_RECTIFY_CHUNK", raising=False)
    else:
        monkeypatch.setenv("PRS_RECTIFY_CHUNK", chunk)  # read per launch: 16 + 16 + 8 images, or 13 chunks of 3 and one of 1
    shape = (33, 65)
    src = image(np.random.default_rng(6), shape, batch=40)
    maps = [make_map("euroc", shape), make_map("strong", shape)]
    map_of = [0] * 20 + [1] * 20  # the switch falls inside a chunk
    check(hip_ctx, ops.rectify_params(), maps, src, map_of=map_of)


# ---- 4. nearest ----
@pytest.mark.parametrize("pixel,np_dtype,border", [("u8", np.uint8, 200), ("u16", np.uint16, 0), ("u16", np.uint16, 65535), ("f32", np.float32, -1.5),
                                                   ("f32", np.float32, float("nan"))], ids=["u8", "u16_0", "u16_65535", "f32", "f32_nan_border"])
def test_nearest(hip_ctx, pixel, np_dtype, border):
    rng = np.random.default_rng(8)
    for shape in ((33, 65), (480, 640)):
        src = image(rng, shape, np_dtype, batch=2)
        if np_dtype == np.float32:  # NaN (with a payload), infinities and a denormal keep their bits
            special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000], dtype=np.uint32).view(np.float32)
            flat = src.reshape(-1)
            flat[rng.choice(flat.size, flat.size // 7, replace=False)] = special[rng.integers(0, len(special), flat.size // 7)]
        P = ops.rectify_params(pixel, "nearest", border)
        assert P.interpolation == ops.RECTIFY_NEAREST
        for kind in ("euroc", "strong"):
            check(hip_ctx, P, [make_map(kind, shape)], src, "nearest", border)
    check(hip_ctx, P, [make_map("euroc", (33, 65))], image(rng, (33, 65), np_dtype, batch=1), "nearest", border, dst_shape=(40, 50), src_pitch=70,
          dst_pitch=51)


# ---- 5. truth without interpolation ambiguity ----
def test_affine_image_against_float64_map(hip_ctx):
    shape = (60, 190)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    a, b, c = 1.0, 1.0, 3.0
    src = (a * xx + b * yy + c).astype(np.uint8)[None]  # at most 251: integer slopes, so bilinear interpolation reproduces it exactly
    m = make_map("euroc", shape)
    got, _, _ = check(hip_ctx, ops.rectify_params(), [m], src)
    us, vs, inside = ref.source_positions(m, shape, shape, np.float64)
    interior = inside & (us >= 0) & (us <= shape[1] - 1) & (vs >= 0) & (vs <= shape[0] - 1)  # every tap inside the source
    want = np.floor(a * us + b * vs + c + 0.5)
    diff = np.abs(got[0].astype(np.float64) - want)[interior]
    share = float(np.count_nonzero(diff)) / diff.size
    print("affine image: %d interior pixels, max %g grey levels off the float64 map, %.4f %% off by one" % (diff.size, diff.max(), 100 * share))
    assert diff.size > 0.8 * shape[0] * shape[1] and diff.max() <= 1 and share <= 0.0015


# ---- 6. chain and capture ----
def test_graph_capture_replays_on_changed_sources(hip_ctx):
    import torch
    shape, B = (60, 190), 6
    rng = np.random.default_rng(10)
    ml, mr = make_map("euroc", shape), make_map("strong", shape)
    frames = [image(rng, shape, batch=B) for _ in range(3)]
    eager = ops.RectifyBatch(hip_ctx, ops.rectify_params(border=4), [ml, mr], B, shape, stereo=True)
    wants = []
    for f in frames:
        wants.append((eager.run(torch.from_numpy(f).cuda()).cpu().numpy().copy(), eager.n_border.cpu().numpy().copy(), eager.status.cpu().numpy().copy()))
    for f, w in zip(frames, wants):  # the eager runs themselves equal the restatement (left block map 0, right block map 1)
        ref_dst, ref_nb, ref_st = ref.rectify_batch(f, [ml, mr], [0] * 3 + [1] * 3, border=4)
        assert same_bits(w[0], ref_dst) and np.array_equal(w[1], ref_nb) and np.array_equal(w[2], ref_st)
    cap = ops.RectifyBatch(hip_ctx, ops.rectify_params(border=4), [ml, mr], B, shape, stereo=True)
    src = torch.from_numpy(frames[0]).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip_ctx.use_torch_stream()
        cap.run(src)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap.run(src)
    torch.cuda.current_stream().wait_stream(s)
    hip_ctx.use_torch_stream()
    for f, w in zip(frames[1:], wants[1:]):
        src.copy_(torch.from_numpy(f))
        cap.dst.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(cap.dst.cpu().numpy(), w[0])
        assert np.array_equal(cap.n_border.cpu().numpy(), w[1]) and np.array_equal(cap.status.cpu().numpy(), w[2])
    assert same_bits(cap.left.cpu().numpy(), wants[2][0][:3]) and same_bits(cap.right.cpu().numpy(), wants[2][0][3:])


def test_extractor_consumes_dst_in_place(hip_ctx):
    import torch
    cfg = configs.EUROC
    left, right, _ = syn.stereo_images(np.random.default_rng(11), cfg)
    src = np.stack([left, right])
    src_shape, dst_shape = src.shape[1:], (480, 750)  # 750 columns in rows of 752 bytes: the extractor reads dst with its pitch
    maps = [make_map("euroc", src_shape, dst_shape), make_map("strong", src_shape, dst_shape)]
    rb = ops.RectifyBatch(hip_ctx, ops.rectify_params(), maps, 2, src_shape, dst_shape, stereo=True)
    dst = rb.run(torch.from_numpy(src).cuda())
    assert dst.stride(1) == 752 and tuple(dst.shape) == (2, 480, 750)
    want, _, _ = ref.rectify_batch(src, maps, [0, 1], dst_shape)
    fresh = torch.from_numpy(want).cuda()
    ep = ops.extractor_params()
    outs = []
    for images in (dst, fresh):
        kp = torch.zeros((2, 4096, 2), dtype=torch.float32, device="cuda")
        desc = torch.zeros((2, 4096, 32), dtype=torch.uint8, device="cuda")
        n = torch.zeros((2,), dtype=torch.int32, device="cuda")
        st = torch.zeros((2,), dtype=torch.int32, device="cuda")
        ops.extract_features_batch(hip_ctx, ep, images, kp, desc, n, st)
        torch.cuda.synchronize()
        outs.append((kp.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()))
    (kp_a, de_a, n_a, st_a), (kp_b, de_b, n_b, st_b) = outs
    assert np.array_equal(n_a, n_b) and np.array_equal(st_a, st_b) and n_a.min() > 100
    for b in range(2):
        assert np.array_equal(kp_a[b, :n_a[b]], kp_b[b, :n_b[b]]) and np.array_equal(de_a[b, :n_a[b]], de_b[b, :n_b[b]])


# ---- 7. refusals: nothing is enqueued, no output is touched ----
def test_call_level_refusals(hip_ctx):
    import torch
    shape = (33, 65)
    m = make_map("euroc", shape).struct()
    d_maps = torch.from_numpy(np.frombuffer((_lib.RectifyMap * 1)(m), dtype=np.uint8).copy()).cuda()
    src = torch.zeros((2, 33, 80), dtype=torch.uint8, device="cuda")
    dst = torch.full((2, 33, 80), PAD, dtype=torch.uint8, device="cuda")
    n_border = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def call(params=None, no_params=False, no_batch=False, **over):
        p = ops.rectify_params() if params is None else params
        d = _lib.RectifyBatch()
        d.batch, d.src_rows, d.src_cols, d.src_pitch, d.src = 2, 33, 65, 80, src.data_ptr()
        d.dst_rows, d.dst_cols, d.dst_pitch, d.dst = 33, 65, 80, dst.data_ptr()
        d.n_maps, d.maps, d.map_of, d.n_border, d.status = 1, d_maps.data_ptr(), None, n_border.data_ptr(), status.data_ptr()
        for k, v in over.items():
            setattr(d, k, v)
        return lib.prs_rectify_batch_run(hip_ctx._h, None if no_params else C.byref(p), None if no_batch else C.byref(d))

    assert call(no_params=True) == ERR_NULL and call(no_batch=True) == ERR_NULL
    for name in ("src", "dst", "maps", "status"):
        assert call(**{name: None}) == ERR_NULL, name
    for over in (dict(batch=0), dict(batch=-3), dict(n_maps=0), dict(src_rows=0), dict(src_cols=0), dict(dst_rows=0), dict(dst_cols=-1),
                 dict(src_pitch=64), dict(dst_pitch=64)):
        assert call(**over) == ERR_RANGE, over
    u16 = ops.rectify_params("u16")
    assert call(u16, src_pitch=131, dst_pitch=132) == ERR_RANGE and call(u16, src_pitch=132, dst_pitch=133) == ERR_RANGE
    assert call(u16, src_pitch=128, dst_pitch=160) == ERR_RANGE  # below 65 * 2
    raw = _lib.RectifyParams
    assert call(raw(3, 1, 0.0, 0)) == ERR_UNSUPPORTED and call(raw(-1, 1, 0.0, 0)) == ERR_UNSUPPORTED  # pixel type
    assert call(raw(0, 2, 0.0, 0)) == ERR_UNSUPPORTED  # interpolation
    assert call(raw(1, 0, 0.0, 0), src_pitch=160, dst_pitch=160) == ERR_UNSUPPORTED  # bilinear for u16
    assert call(raw(2, 0, 0.0, 0), src_pitch=320, dst_pitch=320) == ERR_UNSUPPORTED  # bilinear for f32
    assert call(dst=dst.data_ptr() + 2) == ERR_UNSUPPORTED and call(dst=dst.data_ptr() + 1) == ERR_UNSUPPORTED
    assert call(u16, src=src.data_ptr() + 1, batch=1, src_rows=8, dst_rows=8, src_cols=8, dst_cols=8) == ERR_UNSUPPORTED
    assert call(dst=src.data_ptr()) == ERR_UNSUPPORTED
    assert call(dst=src.data_ptr() + 33 * 80) == ERR_UNSUPPORTED  # the second source image is the first destination image
    assert "overlap" in lib.prs_last_error(hip_ctx._h).decode()
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((n_border == -7).all()) and bool((status == -7).all())
    assert call() == 0  # and the unmodified call runs
    torch.cuda.synchronize()
    assert bool((status == 0).all()) and bool((dst[:, :, 65:] == PAD).all()) and not bool((dst[:, :, :65] == PAD).all())

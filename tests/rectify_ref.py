"""numpy restatement of the image rectifier (include/proslam_hip.h, "Image rectifier"): every operation a two-operand operation of
`dtype` in the order the header writes.  dtype=np.float32 is the parity form, which the kernel equals byte for byte; np.float64 is
the truth the float32 form is judged against.  Also the forward distorted projection of a 3D point and the fixed-point iteration
that inverts the distortion (tests of ops.stereo_rectification)."""
import numpy as np

ERR_RANGE = -4  # PRS_ERR_RANGE
FIELDS = ("src_fx", "src_fy", "src_cx", "src_cy", "k1", "k2", "p1", "p2", "k3", "R", "dst_fx", "dst_fy", "dst_cx", "dst_cy")


def fields(m, dtype=np.float32, exact=False):
    """the map's fields as `dtype` scalars (R: 9 of them, row-major).  m: an ops.RectifyMap or a dict of FIELDS.  The kernel is handed
    float32 values, so they are rounded to float32 first whatever dtype is, unless exact (the host helpers' float64 tests)."""
    if isinstance(m, dict):
        f = {k: np.asarray(m[k], dtype=np.float64) for k in FIELDS}
    else:
        f = dict(src_fx=m.K_src[0, 0], src_fy=m.K_src[1, 1], src_cx=m.K_src[0, 2], src_cy=m.K_src[1, 2], k1=m.dist[0], k2=m.dist[1],
                 p1=m.dist[2], p2=m.dist[3], k3=m.dist[4], R=np.asarray(m.R, dtype=np.float64).reshape(9), dst_fx=m.K_dst[0, 0],
                 dst_fy=m.K_dst[1, 1], dst_cx=m.K_dst[0, 2], dst_cy=m.K_dst[1, 2])
        f = {k: np.asarray(v, dtype=np.float64) for k, v in f.items()}
    f["R"] = f["R"].reshape(9)
    with np.errstate(over="ignore", invalid="ignore"):
        if not exact:
            f = {k: v.astype(np.float32) for k, v in f.items()}
        return {k: v.astype(dtype) for k, v in f.items()}


def map_is_valid(m, model=0):
    """what the kernel checks per image: a known model, every field finite as a float32, no focal length 0"""
    f = fields(m, np.float32)
    finite = all(bool(np.all(np.isfinite(v))) for v in f.values())
    return model == 0 and finite and all(float(f[k]) != 0.0 for k in ("src_fx", "src_fy", "dst_fx", "dst_fy"))


def distort(f, xn, yn):
    """normalised coordinates -> distorted normalised coordinates, in the dtype of the fields"""
    t = xn.dtype.type
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = t(1) + r2 * (f["k1"] + r2 * (f["k2"] + r2 * f["k3"]))
    xd = (xn * rad + (t(2) * f["p1"]) * xy) + f["p2"] * (r2 + t(2) * xx)
    yd = (yn * rad + f["p1"] * (r2 + t(2) * yy)) + (t(2) * f["p2"]) * xy
    return xd, yd


def source_positions(m, dst_shape, src_shape, dtype=np.float32, exact=False):
    """(us, vs, inside) [dst_rows, dst_cols]: where each destination pixel samples the source, and the border rule"""
    f = fields(m, dtype, exact)
    R = f["R"]
    rows, cols = dst_shape
    u = np.broadcast_to(np.arange(cols, dtype=dtype)[None, :], (rows, cols))
    v = np.broadcast_to(np.arange(rows, dtype=dtype)[:, None], (rows, cols))
    with np.errstate(all="ignore"):
        x = (u - f["dst_cx"]) / f["dst_fx"]
        y = (v - f["dst_cy"]) / f["dst_fy"]
        rx = (R[0] * x + R[3] * y) + R[6]
        ry = (R[1] * x + R[4] * y) + R[7]
        rz = (R[2] * x + R[5] * y) + R[8]
        xn, yn = rx / rz, ry / rz
        xd, yd = distort(f, xn, yn)
        us = f["src_fx"] * xd + f["src_cx"]
        vs = f["src_fy"] * yd + f["src_cy"]
        t = np.dtype(dtype).type
        inside = (rz > 0) & (us > t(-1)) & (us < t(src_shape[1])) & (vs > t(-1)) & (vs < t(src_shape[0]))
    assert us.dtype == np.dtype(dtype) and vs.dtype == np.dtype(dtype)
    return us, vs, inside


def border_value(border, np_dtype):
    """params.border in the pixel type, as the library converts it once on the host"""
    if np_dtype == np.float32:
        return np.float32(border)
    top = 255.0 if np_dtype == np.uint8 else 65535.0
    r = np.floor(np.float32(border) + np.float32(0.5))
    return np_dtype(min(r, top)) if r >= 0 else np_dtype(0)


def rectify(src, m, dst_shape=None, interpolation="bilinear", border=0, dtype=np.float32, model=0):
    """one image [rows, cols] of uint8 / uint16 / float32 -> (dst, n_border, status).  An invalid map: all border, PRS_ERR_RANGE."""
    src = np.asarray(src)
    dst_shape = src.shape if dst_shape is None else tuple(dst_shape)
    bv = border_value(border, src.dtype.type)
    if m is None or not map_is_valid(m, model):
        return np.full(dst_shape, bv, dtype=src.dtype), dst_shape[0] * dst_shape[1], ERR_RANGE
    us, vs, inside = source_positions(m, dst_shape, src.shape, dtype)
    rows, cols = src.shape
    t = np.dtype(dtype).type
    n_border = int(np.count_nonzero(~inside))
    us, vs = np.where(inside, us, t(0)), np.where(inside, vs, t(0))  # no float outside the range is converted to an integer
    if interpolation == "nearest":
        xi, yi = np.floor(us + t(0.5)).astype(np.int64), np.floor(vs + t(0.5)).astype(np.int64)
        ok = inside & (xi >= 0) & (xi < cols) & (yi >= 0) & (yi < rows)
        got = src[np.clip(yi, 0, rows - 1), np.clip(xi, 0, cols - 1)]
        return np.where(ok, got, bv).astype(src.dtype), n_border, 0
    assert src.dtype == np.uint8 and interpolation == "bilinear"
    fx0, fy0 = np.floor(us), np.floor(vs)
    ax, ay = us - fx0, vs - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)

    def tap(yy, xx):
        ok = inside & (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
        return np.where(ok, src[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)].astype(dtype), t(bv))

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = a + ax * (b - a)
    bot = c + ax * (d - c)
    val = top + ay * (bot - top)
    assert val.dtype == np.dtype(dtype)
    out = np.minimum(np.maximum(np.floor(val + t(0.5)), t(0)), t(255)).astype(np.uint8)
    return out, n_border, 0


def rectify_batch(srcs, maps, map_of=None, dst_shape=None, interpolation="bilinear", border=0, dtype=np.float32):
    """images [B, rows, cols], maps a list -> (dst [B, ...], n_border [B], status [B]); map_of None: map 0 for every image"""
    out, nb, st = [], [], []
    for b, img in enumerate(srcs):
        i = 0 if map_of is None else int(map_of[b])
        d, n, s = rectify(img, maps[i] if 0 <= i < len(maps) else None, dst_shape, interpolation, border, dtype)
        out.append(d)
        nb.append(n)
        st.append(s)
    return np.stack(out), np.array(nb, np.int32), np.array(st, np.int32)


def project_distorted(m, X, which="src"):
    """float64, exact fields: points X [n, 3] in the raw camera's frame -> their pixels (u, v) [n, 2] in the raw, distorted image
    (which="src"), or X in the rectified camera's frame -> pixels of the rectified image (which="dst": a pinhole)"""
    f = fields(m, np.float64, exact=True)
    X = np.asarray(X, dtype=np.float64)
    xn, yn = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    if which == "dst":
        return np.stack([f["dst_fx"] * xn + f["dst_cx"], f["dst_fy"] * yn + f["dst_cy"]], axis=1)
    xd, yd = distort(f, xn, yn)
    return np.stack([f["src_fx"] * xd + f["src_cx"], f["src_fy"] * yd + f["src_cy"]], axis=1)


def forward_map(m, uv):
    """float64, exact fields: rectified pixels uv [n, 2] -> the raw image's pixels they sample (the kernel's map at real-valued u, v)"""
    f = fields(m, np.float64, exact=True)
    R = f["R"]
    x = (uv[:, 0] - f["dst_cx"]) / f["dst_fx"]
    y = (uv[:, 1] - f["dst_cy"]) / f["dst_fy"]
    rx, ry, rz = (R[0] * x + R[3] * y) + R[6], (R[1] * x + R[4] * y) + R[7], (R[2] * x + R[5] * y) + R[8]
    xd, yd = distort(f, rx / rz, ry / rz)
    return np.stack([f["src_fx"] * xd + f["src_cx"], f["src_fy"] * yd + f["src_cy"]], axis=1)


def undistort_points(m, uv, iterations=40):
    """float64: raw pixels uv [n, 2] -> normalised undistorted coordinates [n, 2], by the fixed-point iteration that inverts the
    radial-tangential model (x <- (x_d - tangential(x)) / radial(x), started at x_d)"""
    f = fields(m, np.float64, exact=True)
    xd = (uv[:, 0] - f["src_cx"]) / f["src_fx"]
    yd = (uv[:, 1] - f["src_cy"]) / f["src_fy"]
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        rad = 1.0 + r2 * (f["k1"] + r2 * (f["k2"] + r2 * f["k3"]))
        dx = 2.0 * f["p1"] * xy + f["p2"] * (r2 + 2.0 * xx)
        dy = f["p1"] * (r2 + 2.0 * yy) + 2.0 * f["p2"] * xy
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return np.stack([x, y], axis=1)

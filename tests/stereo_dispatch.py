"""Plain-Python restatement of the stereo matcher's host dispatch (no GPU needed).

stereo_plan (csrc/stereo_match.hip) refuses a frame shape, takes the layout stereo_v5_layout (csrc/stereo_match_v5.hip) gives it
or carves the LDS of the first-generation kernel; v5 is not taken for shapes whose padded sorted positions or LDS layout do not
fit, nor for distance thresholds above its 8-bit records.  dispatch() says which of the 15 instantiations a
launch reaches (or why it is refused) together with the layout facts the data-dependent paths hang on: v5's `cap`, the pool
offset and `pool_cap`, the first generation's staged / unstaged carve, the grid.  window_demand() counts, per pass of a frame, the
in-window candidates of crowded windows (more than four), which go to the LDS pool until it is full and to the chain's replay
sweep after that.  tests/test_stereo_dispatch_table.py checks dispatch() against the library's own plan (prs_stereo_plan), field
by field over a sweep of shapes and knobs."""
import functools

import numpy as np

KT = 1024               # threads of both matcher kernels (kT, kStereoThreads)
V5_MAX_STRIDE = 2 * KT  # stride > 2 * kT: first generation
V5_CAP_MAX = 8188       # sorted positions are stored in 13 bits
LDS_LIMIT = 160 * 1024
POOL_MIN, POOL_MAX = 64, 4096
V5_BEST_LIM_MAX = 255   # the candidate records keep 8 bits per distance
MAX_STRIDE, MAX_ROWS, MAX_THICKNESS = 8192, 4096, 120
DESC_BYTES = 32
FLT_MAX = np.float32(3.402823466e38)


def _up16(v):
    return (v + 15) & ~15


@functools.lru_cache(maxsize=None)
def accept_limit(max_dist):
    """accept iff best < this: (float) d < maximum_descriptor_distance for integer d"""
    max_dist = np.float32(max_dist)
    lim = 0
    while lim <= 256 and np.float32(lim) < max_dist:
        lim += 1
    return lim


def trace_name(kernel, args):
    """an instantiation (kernel, "KPT,MULTI,EPI" or "KPT,STAGE") as a kernel trace prints it"""
    scope, arg_type = ("prs::v5::", "Args5") if kernel == "stereo_match5_kernel" else ("prs::", "StereoArgs")
    return "void %s%s<%s>(%s%s)" % (scope, kernel, args.replace(",", ", "), scope, arg_type)


TRIANGULATE_KERNEL = "prs::triangulate_kernel(prs_triangulator_params, HIP_vector_type<float, 4u> const*, long, HIP_vector_type<float, 4u>*)"


def fill_accept_table(max_dist, ratio):
    """fill_accept_table: best_lim and bmax[258] from the reference's float operations (epipolar_impl.cpp:171-173)"""
    lim, ratio = accept_limit(max_dist), np.float32(ratio)
    bmax = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(258):
            fs = FLT_MAX if s == 257 else np.float32(s)
            bm = -1
            for b in range(257):
                if np.float32(b) / fs < ratio:
                    bm = b
                elif s != 0:
                    break
            bmax.append(-1 if s == 0 else bm)
    return lim, bmax


def v5_layout(stride, rows):
    """stereo_match_v5_launch's layout: dict(cap, fits, why, lds, off_pool, pool_cap)"""
    cap = (stride + 3 * min(rows, stride) + 3) & ~3
    out = dict(cap=cap, fits=False, why=None, lds=None, off_pool=None, pool_cap=None)
    if cap > V5_CAP_MAX:
        out["why"] = "cap"
        return out
    nwords = (cap + 31) // 32
    rows2 = rows + 2
    off = 0
    for size in (stride * DESC_BYTES, stride * 8, (cap + 4) * 4, (cap + 4) * 4, 2 * (cap + 4) * 4, 2 * rows2 * 4, 2 * rows2 * 2,
                 2 * rows2 * 2, rows2 * 4, cap * 4, nwords * 2 * 4, 32, 258 * 2):
        off = _up16(off + size)
    out["lds"] = off
    if off > LDS_LIMIT:
        out["why"] = "lds"
        return out
    pool_cap = ((LDS_LIMIT - off) // 4) & ~3
    pool_cap = POOL_MAX if pool_cap > POOL_MAX else (0 if pool_cap < POOL_MIN else pool_cap)
    out.update(fits=True, off_pool=off, pool_cap=pool_cap, lds=_up16(off + pool_cap * 4))
    return out


def first_gen_carve(stride, rows, stage):
    """stereo_match_batch_launch's carve lambda: dynamic LDS bytes of the staged / unstaged first-generation kernel"""
    rows1 = rows + 1
    sort_cap = max(stride, rows1)
    nwords = (stride + 31) // 32
    off = 0
    for size in (stride * DESC_BYTES if stage else 0, sort_cap * 4, sort_cap * 4, sort_cap * 8 + 32, (rows1 + 1) * 2, (rows1 + 1) * 2,
                 (rows1 + 1) * 2, nwords * (3 * 4 + 2), 16, 258 * 2, stride * 8 if stage else 0):
        off = _up16(off + size)
    return off


def dispatch(stride, rows, thickness, max_dist, epilogue, matcher_v3=False, force_unstaged=False, batch=1, cus=256):
    """-> dict(kernel, args, refused, v5, staged_lds, unstaged_lds, grid): the instantiation one launch runs.

    kernel / args spell the template as the dispatch does (stereo_match5_kernel "KPT,MULTI,EPI" or stereo_match_kernel
    "KPT,STAGE"); refused is None or the host's reason ("shape", "thickness", "lds"); v5 is v5_layout() when v5 was consulted
    and got as far as its layout."""
    res = dict(kernel=None, args=None, refused=None, v5=None, v5_why=None, staged_lds=None, unstaged_lds=None, grid=0)
    if stride <= 0 or stride > MAX_STRIDE or rows <= 0 or rows > MAX_ROWS:
        res["refused"] = "shape"
        return res
    if thickness > MAX_THICKNESS:
        res["refused"] = "thickness"
        return res
    multi = thickness > 0
    best_lim = accept_limit(max_dist)
    persistent = min(batch, cus)  # one workgroup per CU, frames strided over them
    if stride > V5_MAX_STRIDE or force_unstaged or matcher_v3:
        res["v5_why"] = "knob" if stride <= V5_MAX_STRIDE else "stride"
    else:
        lay = v5_layout(stride, rows)
        res["v5"] = lay
        if not lay["fits"]:
            res["v5_why"] = lay["why"]
        elif best_lim > V5_BEST_LIM_MAX:
            res["v5_why"] = "best_lim"
        else:
            kpt = 1 if stride <= KT else 2
            res["kernel"] = "stereo_match5_kernel"
            res["args"] = "%d,%s,%s" % (kpt, "true" if multi else "false", "true" if epilogue else "false")
            res["grid"] = persistent
            return res
    kpt = 1 if stride <= 1024 else (2 if stride <= 2048 else (4 if stride <= 4096 else 8))
    res["staged_lds"] = first_gen_carve(stride, rows, True)
    res["unstaged_lds"] = first_gen_carve(stride, rows, False)
    stage = not (res["staged_lds"] > LDS_LIMIT or kpt > 2 or force_unstaged)
    if (res["staged_lds"] if stage else res["unstaged_lds"]) > LDS_LIMIT:
        res["refused"] = "lds"
        return res
    res["kernel"] = "stereo_match_kernel"
    res["args"] = "%d,%s" % (kpt, "true" if stage else "false")
    res["grid"] = persistent if stage else batch
    return res


def _features(uv):
    """Feature{row, col, unsorted index} sorted by (row, col, index): epipolar_impl.cpp:8-42 with the canonical tie-break"""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    f = [(int(float(v)), int(float(u)), i) for i, (u, v) in enumerate(uv)]
    f.sort()
    return f


def window_demand(uv_left, uv_right, max_disp, thickness, rows, matched_left_by_pass=None):
    """crowded-window demand of every pass of one frame, as v5's scoring phase sees it.

    A left keypoint on row r scores, in pass o (row offset 0, +1, -1, ..), the right keypoints of row r + offset whose column lies in
    [col - max_disp, col]: every sorted right position counts, pruned or not; a left keypoint matched in an earlier pass does not
    score (matched_left_by_pass: the unsorted left indices matched in each pass, stereo_ref.match(..., passes=True)).
    -> list over passes of dict(windows=[n, ..] (windows of more than four), total=sum, largest=max or 0)."""
    L, R = _features(uv_left), _features(uv_right)
    by_row = {}
    for row, col, _ in R:
        by_row.setdefault(row, []).append(col)
    n_off = 1 + 2 * max(thickness, 0)
    out, done = [], set()
    for o in range(n_off):
        off = 0 if o == 0 else ((o + 1) // 2 if o & 1 else -(o // 2))
        wins = []
        for row, col, idx in L:
            rr = row + off
            if idx in done or rr < 0 or rr >= rows:
                continue
            cols = np.asarray(by_row.get(rr, []))
            n = int(np.count_nonzero((cols >= col - max_disp) & (cols <= col))) if cols.size else 0
            if n > 4:
                wins.append(n)
        out.append(dict(windows=wins, total=sum(wins), largest=max(wins) if wins else 0))
        if matched_left_by_pass is not None and o < len(matched_left_by_pass):
            done |= set(matched_left_by_pass[o])
    return out

"""Plain-Python restatement of the brute-force matcher's host dispatch, bruteforce_plan (csrc/bruteforce.hip); no GPU needed.

dispatch() says which of the 15 kernels a launch reaches (or why it is refused), by the names a kernel trace prints, together with
the facts the data-dependent forks of the kernels hang on: the candidate limit `lim`, the bitmap words `nw`, the candidate capacity
`cap`, the grid, the slices of the split shape (`chunks`), whether the distance bitmaps live in LDS (`bm_fits`), how many candidates
of a pair keep their level lists in LDS (`lvl_cap`), and the dynamic LDS bytes.  tests/test_bruteforce_dispatch_table.py checks
dispatch() against the library's own plan (prs_bruteforce_plan), field by field over a sweep of shapes, modes and switches."""
import functools

import numpy as np

POPCOUNT, MATRIX_WHEN_FULL, MATRIX = 0, 1, 2  # PRS_BF_DENSE_*
FUSED, DENSE, REGISTER = 0, 1, 2             # kBfFused, kBfDense, kBfRegister
THREADS = 1024                               # kBfThreads
LEVELS = 256                                 # kBfLevels
LDS_LIMIT = 160 * 1024
LDS_LIMIT_DUAL = 80 * 1024 - 512
MX_SEG = 192                                 # kMxSeg
PLANE_ROW = 64 + 16                          # kBfmPlaneRow
MFMA_ROWS_WG = 512                           # kBfmRowsWg = 64 rows per wave x 8 waves
MFMA_CHUNK, MFMA_WAVE_LIST, MFMA_FLUSH_AT = 64, 1024, 256  # kBfmChunk, kBfmWaveList, kBfmFlushAt
FULL_BATCH, FULL_FIXED, FULL_MOVING = 32, 256, 64          # the default's switch to the fused matrix shape
SPLIT_MOVING = 256                           # the split shape needs this moving stride (and batch * 2 <= cus)
MAX_FIXED, MAX_MOVING = 8192, 65535
ERR_UNSUPPORTED = -5
REFUSALS = {
    "stride": "prs_bruteforce_match: fixed_stride must be in [1,8192], moving_stride in [1,65535]",
    "threshold": "prs_bruteforce_match: maximum_descriptor_distance above 256 bits",
    "lds": "prs_bruteforce_match: clouds do not fit the 160 KiB LDS",
}


def _up16(v):
    return (v + 15) & ~15


def _up256(v):
    return (v + 255) & ~255


def mx_bytes(threads, chunk):
    """bf_mx_bytes: LDS scratch of the fused shape's matrix-core dense phase"""
    return 2 * 4 * (chunk * PLANE_ROW) + 2 * chunk * 4 + 2 * 16 * 4 + (threads // 64) * MX_SEG * 16


MX_BYTES, MX_BYTES_DUAL = mx_bytes(THREADS, 64), mx_bytes(512, 32)


@functools.lru_cache(maxsize=None)
def limit_of(max_dist):
    """candidate iff d < lim  <=>  (float) d < maximum_descriptor_distance; above LEVELS: refused"""
    max_dist = np.float32(max_dist)
    lim = 0
    with np.errstate(invalid="ignore"):
        while lim <= 257 and np.float32(lim) < max_dist:
            lim += 1
    return lim


def kernel_name(kpt, mode, mx=False, threads=THREADS):
    return "void prs::bruteforce_kernel<%d, %d, %s, %d>(prs::BfArgs)" % (kpt, mode, "true" if mx else "false", threads)


MFMA_KERNEL = "prs::bruteforce_dense_mfma_kernel(prs::BfArgs)"


def all_kernels():
    """the 15 kernels the launch block can reach"""
    names = [kernel_name(k, m) for k in (1, 2, 4, 8) for m in (FUSED, DENSE, REGISTER)]
    return names + [kernel_name(1, FUSED, True), kernel_name(1, FUSED, True, 512), MFMA_KERNEL]


def dispatch(batch, fixed_stride, moving_stride, max_dist, candidate_capacity, mode, cus, env=None):
    """-> dict(refused, kernels, lim, nw, cap, grid, chunks, bm_fits, lvl_cap, fused_matrix, dual, mfma, lds, scratch_bytes)

    mode: the context's PRS_BF_DENSE_* setting; cus: the device's multiProcessorCount; env: the two environment switches
    (PRS_BF_GLOBAL_STATE, PRS_BF_TWO_WORKGROUPS) as a dict of strings."""
    env = env or {}
    res = dict(refused=None, kernels=[], lim=None, nw=None, cap=None, grid=0, chunks=1, bm_fits=None, lvl_cap=0, fused_matrix=False,
               dual=False, mfma=False, lds=0, scratch_bytes=0)
    if batch <= 0:
        return res
    if fixed_stride <= 0 or moving_stride <= 0 or fixed_stride > MAX_FIXED or moving_stride > MAX_MOVING:
        res["refused"] = "stride"
        return res
    lim = limit_of(max_dist)
    if lim > LEVELS:
        res["refused"] = "threshold"
        return res
    nw = (lim + 31) // 32 if lim > 0 else 1
    cap = candidate_capacity if candidate_capacity > 0 else 16 * max(fixed_stride, moving_stride)
    res.update(lim=lim, nw=nw, cap=cap)
    off = 0
    for size in (fixed_stride * 4, moving_stride * 4, fixed_stride, moving_stride, fixed_stride * 4, (4 * LEVELS + 8) * 4):
        off = _up16(off + size)
    if off > LDS_LIMIT:
        res["refused"] = "lds"
        return res
    bm_bytes = (fixed_stride + moving_stride) * nw * 4
    bm_fits = "PRS_BF_GLOBAL_STATE" not in env and off + bm_bytes + 4096 <= LDS_LIMIT
    split_regime = batch * 2 <= cus and moving_stride >= SPLIT_MOVING
    forced, when_full = mode == MATRIX, mode == MATRIX_WHEN_FULL
    fused_matrix = (((forced and not split_regime) or
                     (when_full and batch >= FULL_BATCH and fixed_stride >= FULL_FIXED and moving_stride >= FULL_MOVING)) and
                    bm_fits and _up256(off + bm_bytes) + MX_BYTES <= LDS_LIMIT)
    mfma = not fused_matrix and forced
    two = env.get("PRS_BF_TWO_WORKGROUPS")
    dual = (fused_matrix and ((two[:1] == "1") if two is not None else batch > cus) and
            _up256(off + bm_bytes) + MX_BYTES_DUAL <= LDS_LIMIT_DUAL)
    grid = batch if mfma else (min(batch, 2 * cus) if dual else min(batch, cus))
    chunks = 1
    if mfma:
        chunks = 2
    elif not fused_matrix and split_regime:
        chunks = min(cus // batch, moving_stride // 32)
    lvl_cap = 0
    if bm_fits:
        off = _up16(off + bm_bytes)
        if fused_matrix:
            off = _up256(off)
        room = ((LDS_LIMIT_DUAL if dual else LDS_LIMIT) - off) // 4
        lvl_cap = min(room, cap)
        lists, mx = 4 * lvl_cap, (MX_BYTES_DUAL if dual else MX_BYTES)
        off += mx if fused_matrix and mx > lists else lists
    kpt = (fixed_stride + THREADS - 1) // THREADS
    kpt = 1 if kpt <= 1 else (2 if kpt <= 2 else (4 if kpt <= 4 else 8))
    if chunks > 1:
        kernels = [MFMA_KERNEL if mfma else kernel_name(kpt, DENSE), kernel_name(kpt, REGISTER)]
    elif dual:
        kernels = [kernel_name(1, FUSED, True, 512)]
    elif fused_matrix:
        kernels = [kernel_name(1, FUSED, True)]
    else:
        kernels = [kernel_name(kpt, FUSED)]
    res.update(kernels=kernels, grid=grid, chunks=chunks, bm_fits=bm_fits, lvl_cap=lvl_cap, fused_matrix=fused_matrix, dual=dual,
               mfma=mfma, lds=off, scratch_bytes=grid * cap * 16)
    return res


def split_slices(nm, chunks):
    """[m_begin, m_end) of every workgroup of the split popcount shape (empty slices included)"""
    per = (nm + chunks - 1) // chunks
    return [(c * per, min(c * per + per, nm)) for c in range(chunks)]

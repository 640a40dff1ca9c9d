"""The staging blocks of the host-pointer entry points under reuse: on ONE context every entry point is called with a small
input, then with one large enough to make every block it stages or works in grow, then with the small one again, with
calls of two other entry points in between.  Every result must equal, byte for byte, the result of the same call on a
fresh context: a grown, re-laid-out or shared block must never leak one call's bytes into another's result."""
import numpy as np
import pytest

from srrg2_proslam_amd import configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu

KITTI, ICL = configs.get("kitti"), configs.get("icl")
I4 = np.eye(4, dtype=np.float32)


def _rng(k):
    return np.random.default_rng(syn.seed_for(7, k))


def _stereo(n):
    fr = syn.stereo_frame(_rng(0), KITTI, n)
    sp = ops.stereo_params(KITTI["stereo_matcher"], KITTI["camera"]["rows"])
    return lambda ctx: ops.stereo_match(ctx, sp, fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"])


def _triangulate(n):
    fr = syn.stereo_frame(_rng(1), KITTI, n)
    uvuv = np.concatenate([fr["uv_left"], fr["uv_right"]], axis=1)
    tp = ops.triangulator_params(KITTI)
    return lambda ctx: ops.triangulate(ctx, tp, uvuv)


def _scene_clip(n):
    rng = _rng(2)
    xyzw = np.ones((n, 4), np.float32)
    xyzw[:, :3] = syn.sample_landmarks(rng, KITTI["camera"], KITTI["depth"], n)
    desc = syn.random_descriptors(rng, n)
    R = syn.default_motion(rng, KITTI).astype(np.float32)
    pg = ops.projector_params(KITTI)
    return lambda ctx: ops.scene_clip(ctx, pg, R, I4, xyzw, desc)


def _bruteforce(n):
    rng = _rng(3)
    fixed = syn.random_descriptors(rng, n)
    moving = syn.flip_bits(rng, fixed[rng.permutation(n)[: (3 * n) // 4]], 0.04)
    bp = ops.bruteforce_params()
    return lambda ctx: ops.bruteforce_match(ctx, bp, fixed, moving)


def _selection_order(n):
    response = (syn.random_descriptors(_rng(4), (n + 31) // 32).ravel()[:n] % 255 + 1).astype(np.uint8)
    return lambda ctx: ops.selection_order(ctx, response)


def _image(rows, cols):
    left, _, _ = syn.stereo_images(_rng(5), KITTI)
    return np.ascontiguousarray(left[:rows, :cols])


def _extract(rows, cols, capacity):
    img = _image(rows, cols)
    pg = ops.extractor_params(15, 1, 500, 3, 3, ops.SELECT_LIBSTDCXX, 32768)
    return lambda ctx: ops.extract_features(ctx, pg, img, capacity=capacity)


def _selective(rows, cols, n_proj, capacity):
    img = _image(rows, cols)
    fr = syn.stereo_frame(_rng(6), KITTI, max(n_proj, 1))
    proj = fr["uv_left"][:n_proj] % np.array([cols, rows], np.float32)
    pg = ops.selective_extractor_params("GFTT", "ORB-256", 1000 if n_proj else 100, 10, max_candidates=16384)
    return lambda ctx: ops.extract_features_selective(ctx, pg, img, projections=proj if n_proj else None, radius=10, capacity=capacity)


def _depth(rows, cols, n):
    rng = _rng(7)
    frames, _ = syn.rgbd_image_sequence(rng, ICL, 1)
    depth = np.ascontiguousarray(frames[0][1][:rows, :cols])
    fr = syn.rgbd_frame(rng, ICL, n)
    uv = fr["fixed"][:, :2] % np.array([cols, rows], np.float32)
    inten = rng.uniform(0, 255, n).astype(np.float32)
    dp = ops.depth_params("u16", 0.001)
    return lambda ctx: ops.depth_measurements(ctx, dp, depth, uv, fr["desc_fixed"], inten)


def _point_align(n):
    rng = _rng(8)
    fixed = syn.sample_landmarks(rng, KITTI["camera"], KITTI["depth"], n).astype(np.float32)
    T = syn.default_motion(rng, KITTI)
    moving = ((fixed - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    corr = np.stack([np.arange(n), rng.permutation(n)], axis=1)
    corr[: (4 * n) // 5, 1] = corr[: (4 * n) // 5, 0]
    X0 = syn.perturb(rng, T, 0.05, 0.003)
    pp = ops.point_align_params(KITTI["loop"])
    return lambda ctx: ops.point_align(ctx, pp, fixed, moving, corr, X0)


def _place(n):
    rng = _rng(9)
    base = syn.random_descriptors(rng, n)
    xyz = syn.sample_landmarks(rng, KITTI["camera"], KITTI["depth"], n).astype(np.float32)
    maps = [syn.flip_bits(rng, base, p) for p in (0.02, 0.3, 0.04)]
    query = syn.flip_bits(rng, base, 0.02)
    pp = ops.place_params(KITTI["place"], max_candidates=2, minimum_age_difference_to_candidates=0)

    def run(ctx):
        db = ops.PlaceDatabase(ctx)
        for g, d in enumerate(maps):
            db.add(g, d, xyz=xyz)
        out = db.query(pp, len(maps), query)
        db.close()
        return out

    return run


def _gn_step(k):
    rng = _rng(10 + k)
    A = rng.normal(0, 1, (12, 6))
    H, b = (A.T @ A + np.eye(6)).astype(np.float32), rng.normal(0, 1, 6).astype(np.float32)
    X = syn.perturb(rng, syn.default_motion(rng, KITTI), 0.05, 0.003)
    return lambda ctx: ops.gn_step(ctx, H, b, 1.0, X)


# entry point -> (small call, large call): the large one needs several times the bytes of any small one, in the staging
# block and in every work block its launch takes, so the blocks of a context that has only seen small calls must grow
CALLS = {
    "prs_stereo_match": (lambda: _stereo(64), lambda: _stereo(3000)),
    "prs_triangulate": (lambda: _triangulate(64), lambda: _triangulate(60000)),
    "prs_scene_clip": (lambda: _scene_clip(200), lambda: _scene_clip(60000)),
    "prs_bruteforce_match": (lambda: _bruteforce(96), lambda: _bruteforce(3000)),
    "prs_selection_order": (lambda: _selection_order(96), lambda: _selection_order(32768)),
    "prs_extract_features": (lambda: _extract(96, 160, 512), lambda: _extract(376, 1241, 8192)),
    "prs_extract_features_selective": (lambda: _selective(96, 160, 0, 512), lambda: _selective(376, 1241, 1500, 8192)),
    "prs_depth_measurements": (lambda: _depth(64, 96, 48), lambda: _depth(480, 640, 6000)),
    "prs_point_align": (lambda: _point_align(48), lambda: _point_align(8000)),
    "prs_place_query": (lambda: _place(64), lambda: _place(4000)),
    "prs_gn_step_ex": (lambda: _gn_step(0), lambda: _gn_step(1)),
}
NAMES = list(CALLS)
_cache = {}


def _flat(x):
    if isinstance(x, dict):
        return [b for k in sorted(x) for b in _flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [b for v in x for b in _flat(v)]
    return [b"none" if x is None else np.asarray(x).tobytes()]


def _call(name, size):
    """(the call, its result on a context of its own)"""
    if (name, size) not in _cache:
        f = CALLS[name][size]()
        fresh = ops.Context(0)
        try:
            _cache[(name, size)] = (f, _flat(f(fresh)))
        finally:
            fresh.close()
    return _cache[(name, size)]


def _run_and_compare(ctx, sequence):
    for name, size in sequence:
        f, ref = _call(name, size)
        got = _flat(f(ctx))
        assert len(got) == len(ref) and all(g == r for g, r in zip(got, ref)), (name, "large" if size else "small", sequence)


@pytest.mark.parametrize("name", NAMES)
def test_small_large_small_on_one_context_equals_fresh_contexts(name):
    i = NAMES.index(name)
    a, b = NAMES[(i + 1) % len(NAMES)], NAMES[(i + 5) % len(NAMES)]
    ctx = ops.Context(0)
    try:
        _run_and_compare(ctx, [(name, 0), (a, 0), (name, 1), (b, 0), (name, 0)])
    finally:
        ctx.close()


def test_every_entry_point_in_turn_on_one_context():
    # the same walk with ONE context for all of them: a block grown by one entry point is the next one's to reuse
    ctx = ops.Context(0)
    try:
        for i, name in enumerate(NAMES):
            a, b = NAMES[(i + 2) % len(NAMES)], NAMES[(i + 7) % len(NAMES)]
            _run_and_compare(ctx, [(name, 0), (a, 0), (name, 1), (b, 0), (name, 0)])
    finally:
        ctx.close()

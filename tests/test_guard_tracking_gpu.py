"""The tracking front end inside guard bands (tests/guarded.py): prs_extract_features_batch, prs_extract_features_selective_batch and
prs_align_batch_run in its three modes, at the buffer sizes and alignments include/proslam_hip.h documents for prs_extract_batch,
prs_selective_extract_batch and prs_align_batch.

The cases run the rigs and checkers of the stages' own tests (tests/test_extractor_edges_gpu.py, tests/selective_ref.py,
tests/test_align_dispatch_gpu.py) on arrays carved from an arena: each at exactly the demanded alignment (images at an odd address),
a band of fill bytes on either side, rows from a count to its stride painted with the fill.  B = 3 and the last image or frame is the
full one: its count equals the stride, so its last row adjoins a band.  Each case runs with fill 0x00 and with fill 0xFF on one
oracle evaluation per image or frame: both runs equal the oracle as the stage's own test asserts it, equal each other byte for byte
and leave every band clean.  One case per entry point understates an output's extent by a row, to show that the harness bites, and
one test per pointer whose demand is wider than its element hands in half the demand and is refused with nothing written.

What stays invisible: a read past an array's end whose value reaches no result, and memory the library owns -- the aligner's job
buffers, its lattice and descriptor-row caches and its query cache, the extractors' scratch (responses, masks, candidates, the
smoothed image) -- which cannot be placed."""
import contextlib

import numpy as np
import pytest
import torch

import guarded
import selective_ref as sr
import test_align_dispatch_gpu as dispatch
import test_extractor_edges_gpu as edges
from helpers import aligner_params as oracle_aligner_params, corr_equal, pcf_params_from_cfg
from oracle import binding_features as of
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
B = 3
# the smallest image with an interior tile of fast_blur_kernel, a partial tile on the right and at the bottom, and room inside ORB's
# 31-pixel border on every side
ROWS, COLS = 140, 204
OK, ERR_CAPACITY, ERR_UNSUPPORTED = edges.OK, edges.ERR_CAPACITY, edges.ERR_UNSUPPORTED


# ---- the arrays of the two extractors ------------------------------------------------------------------------------------------------
def put_images(arena, images, pad, name="images"):
    """[B, rows, cols] images in the arena at an odd address, pitch = cols + pad, the padding painted; the array ends at the last pixel
    of the last row.  -> the view the ops wrappers take (its row stride is the pitch)"""
    host = np.stack(images)
    n, rows, cols = host.shape
    big = np.zeros((n, rows, cols + pad), np.uint8)
    big[:, :, :cols] = host
    box = {name: torch.from_numpy(big).to(edges.DEV)}
    t = arena.adopt_pitched(box, name, cols, 1, name=name)
    assert t.data_ptr() % 2 == 1 and t.stride(1) == cols + pad
    return t[:, :, :cols]


def put(arena, name, host, align):
    t = arena.take(host.shape, torch.from_numpy(host).dtype, align, name)
    t.copy_(torch.from_numpy(host))
    return t


def feature_outputs(arena, stride, intensity=True, short=None, tag=""):
    """keypoints, intensity, descriptors, n_features, status, each carved on its own.  short: the name of an array the harness is told
    one row less of"""
    def take(name, shape, dtype, align, row):
        real = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return arena.take(shape, dtype, align, tag + name, extent=real - row if short == name else None)

    kp = take("keypoints", (B, stride, 2), torch.float32, 8, 8)
    inten = take("intensity", (B, stride), torch.float32, 4, 4) if intensity else None
    desc = take("descriptors", (B, stride, 32), torch.uint8, 4, 32)
    n = take("n_features", (B,), torch.int32, 4, 4)
    st = take("status", (B,), torch.int32, 4, 4)
    n.fill_(-7)
    st.fill_(-7)
    return kp, inten, desc, n, st


def features_of(arena, outs):
    """(keypoints, descriptors, intensity, n_features, status) as the edges file's checkers take them; rows from a count to the stride
    still hold the fill: the header says no other row is written"""
    kp, inten, desc, n, st = (None if t is None else t.cpu().numpy() for t in outs)
    for b in range(B):
        k = max(int(n[b]), 0)
        for a in (kp, inten, desc):
            if a is not None:
                assert (a[b, k:].view(np.uint8) == arena.fill).all(), ("a row behind the count was written", b)
    return kp, desc, inten, n, st


def as_dict(out, tag=""):
    return {tag + k: v for k, v in zip(("keypoints", "descriptors", "intensity", "n_features", "status"), out) if v is not None}


# ---- 1. prs_extract_features_batch ------------------------------------------------------------------------------------------------------
def fast_images():
    """dots, coarse texture, fine texture: every image has features, the last one the most"""
    rng = np.random.default_rng(140204)
    pos = edges.lattice(36, ROWS - 36, 36, COLS - 36, 12)
    return [edges.dots(ROWS, COLS, pos, rng.integers(120, 256, len(pos))), edges.smooth_noise(rng, ROWS, COLS, 5), edges.smooth_noise(rng, ROWS, COLS, 3)]


@pytest.fixture
def one_oracle_run(monkeypatch):
    """check_fast asks the oracle once per image and run: the second fill gets the first one's answer"""
    real, memo = of.extract_features, {}

    def once(po, img, capacity=4096):
        key = (bytes(po), img.tobytes(), img.shape, capacity)
        if key not in memo:
            memo[key] = real(po, img, capacity=capacity)
        return memo[key]

    monkeypatch.setattr(of, "extract_features", once)
    return memo


def run_fast(arena, ctx, pg, images, stride, pad, intensity=True, short=None, tag=""):
    img = put_images(arena, images, pad, tag + "images")
    outs = feature_outputs(arena, stride, intensity, short, tag)
    kp, inten, desc, n, st = outs
    ops.extract_features_batch(ctx, pg, img, kp, desc, n, st, inten)
    ctx.synchronize()
    return outs


def fast_counts(po, images):
    return [len(of.extract_features(po, img, capacity=4096)[0]) for img in images]


def test_the_image_reaches_the_paths_it_is_chosen_for():
    t = edges.tiles(ROWS, COLS)
    assert sorted(k for k, inner in t.items() if inner) == [(64, 64), (128, 64)]
    assert any(x0 + 64 > COLS for x0, _ in t) and any(y0 + 64 > ROWS for _, y0 in t)  # partial tiles on the right and at the bottom
    assert min(ROWS, COLS) > 2 * 31 + 64                                                # keypoints on either side of a tile seam
    assert not any(edges.tiles(33, 65).values())


@pytest.mark.parametrize("std", [False, True], ids=["canonical", "libstdcxx"])
@pytest.mark.parametrize("pad", [0, 5], ids=["pitch_cols", "pitch_cols_5"])
def test_extract_features_batch_full_image_at_its_stride(hip_ctx, one_oracle_run, std, pad):
    """stride = the last image's feature count: its last keypoint, intensity and descriptor row adjoin a band; B = 3 below the
    descriptor launch's batch of 8; with intensity and with intensity = NULL"""
    images = fast_images()
    po, pg = edges.fast_params(15, 1, 10 ** 5, (2, 3), std)
    counts = fast_counts(po, images)
    stride = counts[-1]
    assert 0 < min(counts) and max(counts[:-1]) < stride, counts
    assert edges.fast_raw_count(images[-1], 15) <= 8192

    def case(arena):
        out = features_of(arena, run_fast(arena, hip_ctx, pg, images, stride, pad))
        refs = edges.check_fast(po, images, out)
        assert out[3].tolist() == counts and out[3][-1] == out[0].shape[1]
        uv = refs[-1]  # the texture puts keypoints next to every tile seam inside the ORB border
        assert all(np.any(np.abs(uv[:, 0] - seam + 0.5) <= 2.5) for seam in (64, 128)) and np.any(np.abs(uv[:, 1] - 64 + 0.5) <= 2.5)
        bare = features_of(arena, run_fast(arena, hip_ctx, pg, images, stride, pad, intensity=False, tag="bare."))
        assert bare[2] is None
        for name, a, b in zip(("keypoints", "descriptors", "intensity", "n_features", "status"), out, bare):
            assert b is None or a.tobytes() == b.tobytes(), "%s differs without intensity" % name
        return dict(as_dict(out), **as_dict(bare, "bare."))

    guarded.both_fills(case)


def test_extract_features_batch_one_row_short_fails_that_image_alone(hip_ctx, one_oracle_run):
    images = fast_images()
    po, pg = edges.fast_params(15, 1, 10 ** 5, (2, 3), True)
    counts = fast_counts(po, images)
    stride = counts[-1] - 1
    assert 0 < min(counts) and max(counts[:-1]) <= stride

    def case(arena):
        out = features_of(arena, run_fast(arena, hip_ctx, pg, images, stride, 5))
        edges.check_fast(po, images, out, [OK, OK, ERR_CAPACITY])
        return as_dict(out)

    guarded.both_fills(case)


def test_an_understated_descriptor_extent_of_the_extractor_is_reported(hip_ctx):
    images = fast_images()
    po, pg = edges.fast_params(15, 1, 10 ** 5, (2, 3))
    arena = guarded.Arena(0xFF)
    out = features_of(arena, run_fast(arena, hip_ctx, pg, images, fast_counts(po, images)[-1], 0, short="descriptors"))
    assert out[3][-1] == out[0].shape[1]
    with pytest.raises(guarded.Violation, match=r"descriptors after \+0"):
        arena.check()


def offset_view(shape, dtype, nbytes, value):
    """a tensor of this shape whose address is `nbytes` (0 = none) behind a 256-byte boundary, and its whole storage"""
    itemsize = torch.empty((), dtype=dtype).element_size()
    n, skip = int(np.prod(shape)), nbytes // itemsize
    raw = torch.full((n + skip,), value, dtype=dtype, device=edges.DEV)
    view = raw[skip:].view(shape)
    assert raw.data_ptr() % 256 == 0 and view.data_ptr() % 256 == nbytes
    return view, raw


def feature_arguments(which):
    """plain arrays for a refusal test, the one named `which` at half its demand -> (keypoints, descriptors, intensity, n, status), raws"""
    made = [offset_view((B, 8, 2), torch.float32, 4 if which == "keypoints" else 0, -7.0),
            offset_view((B, 8, 32), torch.uint8, 2 if which == "descriptors" else 0, 0x5A),
            offset_view((B, 8), torch.float32, 0, -7.0), offset_view((B,), torch.int32, 0, -7), offset_view((B,), torch.int32, 0, -7)]
    return [v for v, _ in made], [(r, r.clone()) for _, r in made]


def untouched(raws):
    torch.cuda.synchronize()
    return all(torch.equal(now.view(torch.uint8), then.view(torch.uint8)) for now, then in raws)


def refused(message, fn, *args, **kw):
    with pytest.raises(ops.ProslamHipError, match=message) as e:
        fn(*args, **kw)
    assert e.value.status == ERR_UNSUPPORTED


@pytest.mark.parametrize("which", ["keypoints", "descriptors"])
def test_extract_features_batch_refuses_half_the_alignment(hip_ctx, which):
    (kp, desc, inten, n, st), raws = feature_arguments(which)
    img = torch.zeros((B, ROWS, COLS), dtype=torch.uint8, device=edges.DEV)
    _, pg = edges.fast_params()
    refused("keypoints must be 8-byte aligned, descriptors 4-byte", ops.extract_features_batch, hip_ctx, pg, img, kp, desc, n, st, inten)
    assert untouched(raws)


# ---- 2. prs_extract_features_selective_batch ---------------------------------------------------------------------------------------------
def sel_images():
    """texture over 110, 150 and all 204 columns, the rest flat: every image has corners, the last one the most"""
    rng = np.random.default_rng(204140)
    images = [edges.smooth_noise(rng, ROWS, COLS, f) for f in (6, 5, 4)]
    images[0][:, 110:] = 128
    images[1][:, 150:] = 128
    return images


def sel_projections():
    """7, 10 and 16 projections; the last image's fill its row of the array, and four of them have their rectangles clipped at the
    left, right, top and bottom border (two of those at a corner)"""
    rng = np.random.default_rng(7)
    inner = lambda k: np.stack([rng.uniform(40, COLS - 40, k), rng.uniform(40, ROWS - 40, k)], 1).astype(F)  # noqa: E731
    clipped = np.array([(0.0, 70.0), (COLS - 0.5, ROWS - 0.5), (100.0, 0.0), (3.0, ROWS - 1.0)], F)
    return [inner(7), np.concatenate([clipped[:2], inner(8)]), np.concatenate([clipped, inner(12)])]


RADIUS = [2, 0, 5]
SEL_TARGET, SEL_WIDTH = 300, 6
SEL_MODES = ("tracking", "seeding_masked", "seeding_bare")


def sel_case(mode):
    """-> images, projections, radii, masks, pad and the checker's features of every image (the last one the fullest)"""
    images = sel_images()
    proj = radius = masks = None
    pad = 0
    if mode == "tracking":
        proj, radius = sel_projections(), RADIUS
        t = sr.tracking_mask(ROWS, COLS, proj[-1][:4], radius[-1])  # clipped at all four borders
        assert t[:, 0].any() and t[:, -1].any() and t[0].any() and t[-1].any() and not t.all()
        assert len(proj[-1]) == max(len(q) for q in proj)
        refs = [sr.extract(img, SEL_TARGET, SEL_WIDTH, projections=q, radius=r) for img, q, r in zip(images, proj, radius)]
        for img, q, r in zip(images, proj, radius):  # both runs of an image contribute: tracking keypoints, then seeded ones
            t = sr.tracking_mask(ROWS, COLS, q, r)
            assert len(sr.describe(img, sr.gftt(img, t, SEL_TARGET, SEL_WIDTH))[0]) > 0 and len(sr.describe(img, sr.gftt(img, 1 - t, SEL_TARGET, SEL_WIDTH))[0]) > 0
    elif mode == "seeding_masked":
        rng = np.random.default_rng(11)
        masks = [(rng.uniform(size=(ROWS, COLS)) < keep).astype(np.uint8) for keep in (0.4, 0.6, 0.9)]
        for m in masks:
            m[-1, -1] = 1  # the mask's last pixel is one that counts
        pad = 5
        refs = [sr.extract(img, SEL_TARGET, SEL_WIDTH, external_mask=m) for img, m in zip(images, masks)]
    else:
        refs = [sr.extract(img, SEL_TARGET, SEL_WIDTH) for img in images]
    counts = [len(r[0]) for r in refs]
    assert 0 < min(counts) and max(counts[:-1]) < counts[-1], (mode, counts)
    return images, proj, radius, masks, pad, refs, counts


def run_sel(arena, ctx, p, images, stride, pad=0, proj=None, radius=None, masks=None, short=None):
    img = put_images(arena, images, pad)
    kw = {}
    if proj is not None:
        P = len(proj[-1])
        host = np.full((B, P, 2), guarded.host_fill(F, arena.fill), F)  # rows from n_projections[b] to the stride are not read
        for b, q in enumerate(proj):
            host[b, :len(q)] = q
        kw = dict(projections=put(arena, "projections", host, 8), n_projections=put(arena, "n_projections", np.array([len(q) for q in proj], np.int32), 4))
    if radius is not None:
        kw["radius"] = put(arena, "detection_radius", np.array(radius, np.int32), 4)
    if masks is not None:
        kw["seeding_mask"] = put_images(arena, masks, pad, "seeding_mask")
    outs = feature_outputs(arena, stride, True, short)
    kp, inten, desc, n, st = outs
    ops.extract_features_selective_batch(ctx, p, img, kp, desc, n, st, inten, **kw)
    ctx.synchronize()
    return outs


@pytest.mark.parametrize("mode", SEL_MODES)
def test_extract_features_selective_batch_full_image_at_its_stride(hip_ctx, mode):
    """tracking: projections at their stride, a radius per image, seeding when tracking on, rectangles clipped at all four borders;
    seeding inside a pitched mask that ends at its last pixel; seeding with every optional pointer NULL"""
    images, proj, radius, masks, pad, refs, counts = sel_case(mode)
    p = edges.sel_params(SEL_TARGET, SEL_WIDTH)

    def case(arena):
        out = features_of(arena, run_sel(arena, hip_ctx, p, images, counts[-1], pad, proj, radius, masks))
        edges.check_sel(out, refs)
        assert out[3][-1] == out[0].shape[1]
        return as_dict(out)

    guarded.both_fills(case)


def test_extract_features_selective_batch_one_row_short_fails_that_image_alone(hip_ctx):
    images, proj, radius, masks, pad, refs, counts = sel_case("tracking")
    assert max(counts[:-1]) <= counts[-1] - 1
    p = edges.sel_params(SEL_TARGET, SEL_WIDTH)

    def case(arena):
        out = features_of(arena, run_sel(arena, hip_ctx, p, images, counts[-1] - 1, 5, proj, radius))
        edges.check_sel(out, refs, [OK, OK, ERR_CAPACITY])
        return as_dict(out)

    guarded.both_fills(case)


def test_an_understated_descriptor_extent_of_the_selective_extractor_is_reported(hip_ctx):
    images, proj, radius, masks, pad, refs, counts = sel_case("seeding_bare")
    arena = guarded.Arena(0xFF)
    out = features_of(arena, run_sel(arena, hip_ctx, edges.sel_params(SEL_TARGET, SEL_WIDTH), images, counts[-1], short="descriptors"))
    assert out[3][-1] == out[0].shape[1]
    with pytest.raises(guarded.Violation, match=r"descriptors after \+0"):
        arena.check()


@pytest.mark.parametrize("which", ["keypoints", "descriptors", "projections"])
def test_extract_features_selective_batch_refuses_half_the_alignment(hip_ctx, which):
    (kp, desc, inten, n, st), raws = feature_arguments(which)
    img = torch.zeros((B, ROWS, COLS), dtype=torch.uint8, device=edges.DEV)
    proj, _ = offset_view((B, 4, 2), torch.float32, 4 if which == "projections" else 0, 50.0)
    counts = torch.full((B,), 4, dtype=torch.int32, device=edges.DEV)
    refused("keypoints and projections must be 8-byte aligned, descriptors 4-byte", ops.extract_features_selective_batch, hip_ctx,
            edges.sel_params(), img, kp, desc, n, st, inten, projections=proj, n_projections=counts)
    assert untouched(raws)


# ---- 3. prs_align_batch_run ------------------------------------------------------------------------------------------------------------------
ALIGNS = dict(fixed=16, moving=16, fixed_desc=16, moving_desc=16, state=8, result=4)  # (the other arrays: their element, guarded.row_align)
ARRAYS = ("fixed", "fixed_desc", "n_fixed", "moving", "moving_desc", "n_moving", "inputs_changed", "state", "X", "corr", "n_corr", "result")
OUTPUTS = ("X", "corr", "n_corr", "state", "result")
ROW = {r["id"]: r for r in dispatch.DISPATCH}


@contextlib.contextmanager
def guarded_frames(arena, monkeypatch, made, short_corr=False):
    """every ops.AlignFrames built inside moves into the arena, rows of fixed, fixed_desc, moving, moving_desc and corr painted (upload
    writes the first n of them); prior_mean, which the dispatch rig attaches after construction, follows at the call.  short_corr: the
    harness is told one row less of corr"""
    def slack(f):
        if short_corr:
            arena.adopt(f, "corr", 4, extent=f.corr.numel() * 4 - 12, name="corr.short")
        for t in (f.fixed, f.fixed_desc, f.moving, f.moving_desc, f.corr):
            arena.paint(t)
        made.append(f)

    real = ops.align_batch

    def align_batch(ctx, fp, ap, frames, mode=_lib.MODE_ALIGN):
        for k in ("prior", "prior_mean"):
            if getattr(frames, k) is not None and not arena.owns(getattr(frames, k)):
                arena.adopt(frames, k, 4, name="AlignFrames." + k)
        return real(ctx, fp, ap, frames, mode)

    with monkeypatch.context() as m:
        m.setattr(ops, "align_batch", align_batch)
        with guarded.hooked(arena, ops.AlignFrames, aligns=ALIGNS, after=slack):
            yield


def frames_out(arena, made, full=True):
    """the one batch of the case: all of it in the arena; the last frame the full one; corr rows from n_fixed[b] on still the fill"""
    f, = made
    names = ARRAYS + tuple(k for k in ("prior", "prior_mean") if getattr(f, k) is not None)
    assert all(arena.owns(getattr(f, k)) for k in names)
    for k, a in ALIGNS.items():
        assert getattr(f, k).data_ptr() % (2 * a) == a, k
    n_fixed, n_moving = f.n_fixed.tolist(), f.n_moving.tolist()
    if full:
        assert n_fixed[-1] == f.fixed_stride == (f.max_fixed or f.fixed_stride) and n_moving[-1] == f.moving_stride == max(n_moving), (n_fixed, n_moving)
    corr = f.corr.cpu().numpy()
    for b in range(f.batch):
        assert (corr[b, n_fixed[b]:].view(np.uint8) == arena.fill).all(), ("a correspondence row behind n_fixed was written", b)
    return {k: getattr(f, k).cpu().numpy() for k in OUTPUTS}


@pytest.fixture
def one_oracle_frame(monkeypatch):
    """the dispatch rig asks the oracle once per frame and run: the second fill gets the first one's answer"""
    real, memo = dispatch._oracle_frame, {}

    def once(oracle, cfg, c, *a, **kw):
        if id(c) not in memo:
            memo[id(c)] = (c, real(oracle, cfg, c, *a, **kw))
        return memo[id(c)][1]

    monkeypatch.setattr(dispatch, "_oracle_frame", once)
    return memo


def row_cases(oracle, row, n=B):
    """the frames the dispatch test runs for this row, the full one last"""
    cfg, cases = dispatch._cases(row["cfg"], 7100 + 13 * dispatch.DISPATCH.index(row), n, row["max_fixed"], full=1)
    cases = cases[::-1]
    for c in cases:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
        if row.get("sensor"):
            c["X0"] = (dispatch.SENSOR.astype(np.float64) @ c["X0"]).astype(F)
    assert len(cases[-1]["fixed"]) == row["max_fixed"] and len(cases[-1]["xyz"]) == max(len(c["xyz"]) for c in cases)
    return cfg, cases


def test_the_rows_cover_what_the_issue_names():
    rows = dispatch.DISPATCH
    assert {(r["cfg"], r["max_fixed"]) for r in rows} >= {("kitti", 512), ("kitti", 600), ("tum", 512), ("euroc", 512)}
    assert {"tp4_plain", "five_plain", "depth4", "generic4", "lone8_sensor", "lone4_mprior", "fused_forced", "fused_by_size"} <= set(ROW)
    assert any(r.get("sensor") for r in rows) and any(r.get("mprior") for r in rows)


@pytest.mark.parametrize("row", dispatch.DISPATCH, ids=[r["id"] for r in dispatch.DISPATCH])
def test_align_batch_run_every_row_with_the_full_frame_last(oracle, monkeypatch, one_oracle_frame, row):
    """every instantiation of the dispatch: n_fixed == max_fixed == fixed_stride and n_moving == moving_stride in the last frame, each
    frame against the oracle and the float64 step as the dispatch test asserts them"""
    cfg, cases = row_cases(oracle, row)
    ctx = dispatch._context(monkeypatch, no_lone=row["no_lone"], fused=row.get("fused", 0))

    def case(arena):
        made = []
        with guarded_frames(arena, monkeypatch, made):
            n_corr, converged = dispatch._row_parity(oracle, ctx, row, cases, cfg)
        assert max(n_corr) > 100 and converged >= 1, (n_corr, converged)
        assert (made[0].prior_mean is not None) == bool(row.get("mprior"))
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
    finally:
        ctx.close()
    assert len(one_oracle_frame) == B


def test_align_batch_run_with_an_external_prior(oracle, monkeypatch, one_oracle_frame):
    """prior [batch][42] and prior_mean [batch][16] in bands of their own: an externally linearised slice on top of the motion prior"""
    row = ROW["lone4_mprior"]
    cfg, cases = row_cases(oracle, row)
    rng = np.random.default_rng(42)
    for c in cases:
        c["prior"] = ((np.eye(6) * rng.uniform(1, 20)).astype(F), rng.normal(0, 0.5, 6).astype(F))
    ctx = dispatch._context(monkeypatch, no_lone=row["no_lone"])
    fkw = row["fkw"]

    def case(arena):
        made = []
        with guarded_frames(arena, monkeypatch, made):
            frames = ops.AlignFrames(0, B, row["max_fixed"], max(len(c["xyz"]) for c in cases), with_prior=True)
            frames.max_fixed = row["max_fixed"]
            for b, c in enumerate(cases):
                frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])
                frames.prior[b] = torch.from_numpy(np.concatenate([c["prior"][0].ravel(), c["prior"][1]])).cuda()
            frames.prior_mean = torch.from_numpy(np.stack([c["X0"].reshape(16) for c in cases]).astype(F)).cuda()
            dispatch._run_batch(ctx, cfg, cases, row["max_fixed"], fkw, {}, mprior=True, frames=frames, expect=dispatch.row_kernels(row))
        for b, c in enumerate(cases):
            ofr, res, rcorr = dispatch._oracle_frame(oracle, cfg, c, fkw, {}, mprior=True, prior=c["prior"])
            dispatch._check_frame(frames, b, ofr, res, rcorr, "prior frame %d" % b)
        assert arena.owns(frames.prior) and arena.owns(frames.prior_mean)
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
    finally:
        ctx.close()


def finder_refs(oracle, cfg, cases, fkw):
    """one CorrespondenceFinderProjective::compute() per frame with local_map_in_sensor = the frame's guess"""
    out = []
    for c in cases:
        f = oracle.ProjectiveFinder(pcf_params_from_cfg(oracle, cfg, **fkw))
        f.set_fixed(c["fixed"], c["dfix"])
        f.set_moving(c["xyz"], c["dmov"])
        f.set_local_map_in_sensor(c["X0"])
        corr, flags = f.compute()
        out.append((f, corr, flags))
    return out


def build_frames(cases, stride):
    frames = ops.AlignFrames(0, len(cases), stride, max(len(c["xyz"]) for c in cases))
    frames.max_fixed = stride
    for b, c in enumerate(cases):
        frames.upload(b, c["fixed"], c["dfix"], c["xyz"], c["scale"], c["dmov"], c["X0"])
    return frames


def check_finder(frames, refs):
    """what tests/test_finder_aligner_gpu.py compares call by call: correspondences, flags and the finder's state"""
    for b, (f, corr, flags) in enumerate(refs):
        st, res = frames.state_of(b), frames.result_of(b)
        assert corr_equal(corr, frames.corr_of(b)), "frame %d: %d vs %d correspondences" % (b, len(corr), int(frames.n_corr[b]))
        assert res.warnings == flags, (b, res.warnings, flags)
        assert (f.search_radius, f.iteration, f.has_converged, f.num_recomputes) == (int(st.search_radius_pixels), int(st.current_iteration), bool(st.has_converged), int(st.num_recomputes)), b
        assert np.float32(f.descriptor_distance) == np.float32(st.descriptor_distance), b
        assert np.array_equal(dispatch._bits(f.local_map_in_sensor()).ravel(), dispatch._bits(np.array(st.local_map_in_sensor))), b


def test_align_batch_run_finder_mode(oracle, monkeypatch):
    row = ROW["lone4_plain"]
    cfg, cases = row_cases(oracle, row)
    refs = finder_refs(oracle, cfg, cases, row["fkw"])
    assert min(len(r[1]) for r in refs) > 50
    fp, ap = dispatch._device_params(cfg, row["fkw"], {})
    ctx = dispatch._context(monkeypatch)

    def case(arena):
        made = []
        with guarded_frames(arena, monkeypatch, made):
            frames = build_frames(cases, row["max_fixed"])
            ops.align_batch(ctx, fp, ap, frames, _lib.MODE_FINDER)
        torch.cuda.synchronize()
        check_finder(frames, refs)
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
    finally:
        ctx.close()


def test_align_batch_run_linearize_mode(oracle, monkeypatch):
    """corr is an input: the finder's correspondences, filled up to n_corr == fixed_stride with further pairs in the full frame.
    H, b, the class counts and the chi sums as tests/test_finder_aligner_gpu.py::test_linearize_is_bit_exact compares them"""
    row = ROW["lone4_plain"]
    cfg, cases = row_cases(oracle, row)
    rng = np.random.default_rng(512)
    corrs, refs = [], []
    for b, (c, (f, corr, flags)) in enumerate(zip(cases, finder_refs(oracle, cfg, cases, row["fkw"]))):
        if b == B - 1:
            more = np.zeros(row["max_fixed"] - len(corr), dtype=corr.dtype)
            more["fixed_idx"], more["moving_idx"] = rng.integers(0, len(c["fixed"]), len(more)), rng.integers(0, len(c["xyz"]), len(more))
            corr = np.concatenate([corr, more])
        oap = oracle_aligner_params(oracle, cfg, mean_disparity=oracle.mean_disparity(c["fixed"]))
        corrs.append(corr)
        refs.append(oracle.linearize(oap, c["X0"], corr, c["fixed"], c["xyz"], c["scale"]))
    assert len(corrs[-1]) == row["max_fixed"] and min(len(c) for c in corrs) > 50 and refs[-1].num_outliers > 0
    fp, ap = dispatch._device_params(cfg, row["fkw"], {})
    ctx = dispatch._context(monkeypatch)

    def case(arena):
        made = []
        with guarded_frames(arena, monkeypatch, made):
            frames = build_frames(cases, row["max_fixed"])
            given = []
            for b, corr in enumerate(corrs):
                raw = np.stack([corr["fixed_idx"], corr["moving_idx"], corr["response"].view(np.int32)], 1).astype(np.int32)
                frames.corr[b, :len(raw)] = torch.from_numpy(raw).cuda()
                frames.n_corr[b] = len(raw)
                given.append(raw)
            ops.align_batch(ctx, fp, ap, frames, _lib.MODE_LINEARIZE)
        torch.cuda.synchronize()
        assert frames.n_corr.tolist() == [len(g) for g in given] and frames.n_corr.tolist()[-1] == frames.fixed_stride
        for b, (ref, raw) in enumerate(zip(refs, given)):
            got = frames.result_of(b)
            assert np.array_equal(frames.corr[b, :len(raw)].cpu().numpy(), raw), b  # an input: left as it was
            assert np.array_equal(dispatch._bits(np.array(ref.H)), dispatch._bits(np.array(got.H))), b
            assert np.array_equal(dispatch._bits(np.array(ref.b)), dispatch._bits(np.array(got.b))), b
            assert (ref.num_inliers, ref.num_outliers, ref.num_invalid) == (got.num_inliers, got.num_outliers, got.num_invalid), b
            assert np.float32(ref.chi_inliers) == np.float32(got.chi_inliers) and np.float32(ref.chi_total) == np.float32(got.chi_total), b
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
    finally:
        ctx.close()


# ---- the pruned scan's entry behind the last one ----------------------------------------------------------------------------------------------
def sentinel_cases(cfg):
    """correlated frames of 500, 600 and 700 points; the last is full, its last fixed row sits in the canvas' last pixel -- the last
    cell a scan visits -- and shares its descriptor with the row before it"""
    rng = np.random.default_rng(602)
    cases = [dispatch._correlated_frame(rng, cfg, n, corner=(n == 700)) for n in (500, 600, 700)]
    last = cases[-1]
    last["dfix"][-2] = last["dfix"][-1]
    uv, cam = last["fixed"][:, :2], cfg["camera"]
    assert tuple(uv[-1]) == (cam["cols"] - 1, cam["rows"] - 1) and uv[:, 1].max() == uv[-1, 1] and uv[uv[:, 1] == uv[-1, 1], 0].max() == uv[-1, 0]
    assert np.array_equal(last["dfix"][-2], last["dfix"][-1]) and len(last["fixed"]) == 700 == max(len(c["xyz"]) for c in cases)
    return cases


@pytest.mark.parametrize("fused", [0, 1], ids=["split", "fused"])
def test_align_batch_run_last_entry_of_a_full_frame_in_the_last_scanned_cell(oracle, monkeypatch, one_oracle_frame, fused):
    """nF == max_fixed == fixed_stride: row nF of fixed_desc is the band.  The scan's one entry past a segment must be the sentinel in
    LDS; were it the caller's row nF and did it reach a survivor, the result would move between the fills"""
    cfg = configs.get("kitti")
    cases = sentinel_cases(cfg)
    row = dict(id="sentinel", max_fixed=700, fkw=dict(search_type=2, maximum_search_radius_pixels=100))
    ctx = dispatch._context(monkeypatch, fused=fused)

    def case(arena):
        made = []
        with guarded_frames(arena, monkeypatch, made):
            n_corr, _ = dispatch._row_parity(oracle, ctx, row, cases, cfg)
        assert sum(n_corr) > 150, n_corr
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
    finally:
        ctx.close()


# ---- the harness bites, and the launcher refuses ---------------------------------------------------------------------------------------------
def matched_frame(rng, cfg, n):
    """a stereo frame in which every fixed point has its moving point: the same points shuffled, the same descriptors, a guess next to
    the truth; one compute() gives n correspondences, the whole of corr"""
    cam = cfg["camera"]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    i = np.arange(n)
    uv = np.stack([300 + 40 * (i % 16), 40 + 24 * (i // 16)], 1).astype(F)
    depth = rng.uniform(6.0, 40.0, n).astype(F)
    xyz = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], 1).astype(F)
    disparity = (fx * cam["baseline_m"] / depth).astype(F)
    fixed = np.concatenate([uv, uv - np.stack([disparity, np.zeros(n, F)], 1)], 1).astype(F)
    dfix = syn.random_descriptors(rng, n)
    order = rng.permutation(n)
    return dict(fixed=fixed, dfix=dfix, xyz=xyz[order].copy(), dmov=dfix[order].copy(), scale=None, X0=syn.perturb(rng, np.eye(4), 0.02, 0.001))


def matched_cases(cfg):
    rng = np.random.default_rng(64)
    return [matched_frame(rng, cfg, n) for n in (40, 50, 64)]


def test_align_batch_run_a_correspondence_per_fixed_point(oracle, monkeypatch):
    """n_corr == n_fixed == fixed_stride in the last frame: the last row of corr is written and adjoins a band.  Once more with corr
    believed a row shorter: the harness reports that row"""
    cfg = configs.get("kitti")
    cases = matched_cases(cfg)
    refs = finder_refs(oracle, cfg, cases, {})
    assert [len(r[1]) for r in refs] == [40, 50, 64]
    fp, ap = dispatch._device_params(cfg, {}, {})
    ctx = dispatch._context(monkeypatch)

    def case(arena, short=False):
        made = []
        with guarded_frames(arena, monkeypatch, made, short_corr=short):
            frames = build_frames(cases, 64)
            ops.align_batch(ctx, fp, ap, frames, _lib.MODE_FINDER)
        torch.cuda.synchronize()
        check_finder(frames, refs)
        assert frames.n_corr.tolist()[-1] == frames.fixed_stride
        return frames_out(arena, made)

    try:
        guarded.both_fills(case)
        arena = guarded.Arena(0xFF)
        case(arena, short=True)
        with pytest.raises(guarded.Violation, match=r"corr\.short after \+0"):
            arena.check()
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["fixed", "moving", "fixed_desc", "moving_desc"])
def test_align_batch_run_refuses_half_the_alignment(hip_ctx, which):
    cfg = configs.get("kitti")
    cases = matched_cases(cfg)
    frames = build_frames(cases, 64)
    old = getattr(frames, which)
    view, _ = offset_view(tuple(old.shape), old.dtype, 8, 0)
    view.copy_(old)
    setattr(frames, which, view)
    for k, v in (("X", -7.0), ("corr", -7), ("n_corr", -7), ("result", 0x5A)):
        getattr(frames, k).fill_(v)
    raws = [(getattr(frames, k), getattr(frames, k).clone()) for k in OUTPUTS]
    fp, ap = dispatch._device_params(cfg, {}, {})
    for mode in (_lib.MODE_ALIGN, _lib.MODE_FINDER, _lib.MODE_LINEARIZE):
        refused("fixed, moving, fixed_desc and moving_desc must be 16-byte aligned", ops.align_batch, hip_ctx, fp, ap, frames, mode)
    assert untouched(raws)

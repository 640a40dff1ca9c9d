"""The speckle filter on the device (ops.SpeckleFilterBatch: prs_speckle_batch_run) against its numpy restatement
(tests/speckle_ref.py).  Every array is compared byte for byte over its whole allocated length: every decision of the rule is exact,
so no tolerance is involved; pad columns and the images a call must not touch are compared with what they held (image, companion) or
with the sentinel they were filled with (label, the counts, status).  The tile kernel's workgroup owns a TW x TH tile of an image; the
seam kernel joins the tiles across their borders; a flatten or apply workgroup owns CHUNK pixels of an image's raster."""
import ctypes as C

import numpy as np
import pytest

import speckle_ref as ref
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
TW, TH = 64, 16
CHUNK = 2048  # pixels of a flatten or apply workgroup
INF, NAN = F(np.inf), F(np.nan)
TORCH = {np.dtype(np.float32): "float32", np.dtype(np.uint16): "uint16"}
TYPE = {np.dtype(np.float32): "f32", np.dtype(np.uint16): "u16"}


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def padded(host, pad):
    """host [..., cols] with `pad` elements behind every row that look valid and would connect if they were read: the row's last
    element, or 1 where that is not valid"""
    if pad == 0:
        return host.copy()
    last = host[..., -1:]
    with np.errstate(invalid="ignore"):
        fill = np.where(last > 0, last, host.dtype.type(1))
    return np.concatenate([host, np.repeat(fill, pad, axis=-1)], axis=-1)


class Rig:
    """an ops.SpeckleFilterBatch over device copies of images (and companions) [B, frames, rows, cols], float32 or uint16.  pad:
    elements behind every row of image, companion (pad + 1) and so a pitch above cols; flat: the tensors go in as
    [B * frames, rows, cols]"""

    def __init__(self, ctx, images, companions=None, n_images=None, pad=0, outputs=ops.SpeckleFilterBatch.OUTPUTS, flat=False):
        import torch
        self.ctx, self.pad, self.flat = ctx, pad, flat
        self.B, self.frames, self.rows, self.cols = images.shape
        self.dev = torch.device("cuda", 0)
        self.sf = ops.SpeckleFilterBatch(self.B, self.frames, self.rows, self.cols, outputs)
        full = lambda host, extra: torch.zeros(host.shape[:3] + (self.cols + extra,), dtype=getattr(torch, TORCH[host.dtype]), device=self.dev)  # noqa: E731
        self.t_image = full(images, pad)
        self.t_companion = full(companions, pad + 1 if pad else 0) if companions is not None else None
        self.t_n = torch.zeros((self.B,), dtype=torch.int32, device=self.dev) if n_images is not None else None
        self.types = dict(pixel_type=TYPE[images.dtype], companion_type=TYPE[companions.dtype] if companions is not None else None)
        self.upload(images, companions, n_images)

    def upload(self, images, companions=None, n_images=None):
        import torch
        self.images, self.companions, self.n_images = images, companions, n_images
        self.full_image = padded(images, self.pad)
        self.t_image.copy_(torch.from_numpy(self.full_image))
        if companions is not None:
            self.full_companion = padded(companions, self.pad + 1 if self.pad else 0)
            self.t_companion.copy_(torch.from_numpy(self.full_companion))
        if n_images is not None:
            self.t_n.copy_(torch.tensor(n_images, dtype=torch.int32))

    def inputs(self):
        view = lambda t: None if t is None else (t.flatten(0, 1) if self.flat else t)[..., :self.cols]  # noqa: E731
        return dict(image=view(self.t_image), companion=view(self.t_companion), n_images=self.t_n)

    def tensors(self):
        out = dict(image=self.t_image, companion=self.t_companion, label=self.sf._label, n_kept=self.sf.n_kept, n_removed=self.sf.n_removed,
                   status=self.sf.status)
        return {k: t for k, t in out.items() if t is not None}

    def fill_sentinel(self):
        import torch
        for k, t in self.tensors().items():
            if k not in ("image", "companion"):
                t.view(torch.uint8).fill_(SENTINEL)

    def outputs(self):
        return {k: t.cpu().numpy() for k, t in self.tensors().items()}

    def expected(self, rp):
        """every array as the call must leave it, the int32 ones from a sentinel-filled state, and the restatement's results"""
        want = {k: np.full(tuple(t.shape), SENTINEL, np.uint8).repeat(4, axis=-1).view(np.int32)
                for k, t in self.tensors().items() if k not in ("image", "companion")}
        want["image"] = self.full_image.copy()
        if self.companions is not None:
            want["companion"] = self.full_companion.copy()
        results = []
        for b in range(self.B):
            n = None if self.n_images is None else self.n_images[b]
            r = ref.speckle(self.images[b], None if self.companions is None else self.companions[b], n, rp)
            results.append(r)
            want["status"][b] = r["status"]
            for f, image in enumerate(r["results"]):
                if image is not None:
                    for k in ("image", "companion", "label"):
                        if k in want:
                            want[k][b, f, :, :self.cols] = image[k]
                    for k in ("n_kept", "n_removed"):
                        if k in want:
                            want[k][b, f] = image[k]
        return want, results

    def compare(self, got, want, what=""):
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(got[k].view(np.uint8) != want[k].view(np.uint8))[:5])

    def check(self, max_size, max_diff=1.0, what=""):
        """upload the input again (the call works in place), run, compare with the restatement; -> its results per sequence"""
        p = ops.speckle_params(max_size, max_diff, **self.types)
        self.upload(self.images, self.companions, self.n_images)
        self.fill_sentinel()
        self.sf.run(self.ctx, p, **self.inputs())
        self.ctx.synchronize()
        want, results = self.expected(ref.params(max_size, max_diff))
        self.compare(self.outputs(), want, (what, max_size, max_diff))
        return results


def images_of(results):
    return [image for r in results for image in r["results"] if image is not None]


def one(image):
    return np.ascontiguousarray(image)[None, None]


def noise(rng, shape, density, levels=3, dtype=np.float32):
    """quantised noise: `levels` values a step of 1 apart, a pixel valid with probability `density`"""
    return (rng.integers(1, levels + 1, shape) * (rng.random(shape) < density)).astype(dtype)


# ---- 1. tile geometry ----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, TW + 5), (TH + 5, 1), (TH - 1, TW - 1), (TH, TW - 1), (TH - 1, TW), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 3),
          (3, 2 * TW + 2), (CHUNK // TW, TW), (23, 89), (3, 683)]
assert 23 * 89 == CHUNK - 1 and 3 * 683 == CHUNK + 1


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(hip_ctx, shape, dtype):
    rig = Rig(hip_ctx, noise(_rng(1, *shape), (2, 2) + shape, 0.62, dtype=dtype))
    results = rig.check(4)
    assert shape[0] * shape[1] < 100 or sum(i["n_removed"] for i in images_of(results)) > 0
    rig.check(2 ** 31 - 1, 0.0)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
@pytest.mark.parametrize("pad", [1, 3, 32])
def test_a_pitch_above_cols(hip_ctx, pad, dtype):
    """the pad elements repeat the row's last pixel: read as a neighbour they would lengthen its component"""
    shape = (2, 2, TH + 2, TW + 3)
    images = noise(_rng(2, pad), shape, 0.7, dtype=dtype)
    images[..., -1] = 2  # a valid last column whose component a pad element would join
    companions = noise(_rng(2, pad, 1), shape, 0.9, 5, np.float32) + F(0.5)
    rig = Rig(hip_ctx, images, companions, pad=pad)
    assert rig.inputs()["image"].stride(2) == TW + 3 + pad and rig.inputs()["companion"].stride(2) == TW + 4 + pad
    for max_size in (0, 3, TH + 2, 40):
        rig.check(max_size)


# ---- 2. seams ------------------------------------------------------------------------------------------------------------------------
def test_a_block_on_the_corner_of_four_tiles(hip_ctx):
    image = np.zeros((2 * TH, 2 * TW), F)
    image[TH - 1:TH + 1, TW - 1:TW + 1] = 3
    rig = Rig(hip_ctx, one(image))
    for max_size, removed in ((3, 0), (4, 4)):
        r = images_of(rig.check(max_size))[0]
        assert r["n_removed"] == removed and r["label"][TH, TW] == (TH - 1) * 2 * TW + TW - 1


@pytest.mark.parametrize("n", [5, 6])
def test_components_of_max_size_and_one_more_across_seams(hip_ctx, n):
    """bars of n and n + 1 pixels across a vertical and across a horizontal seam, and an L around the corner: max_size = n removes the
    bars of n pixels only"""
    image = np.zeros((2 * TH + 2, 2 * TW + 2), np.uint16)
    image[3, TW - 2:TW - 2 + n] = 7          # across the vertical seam
    image[7, TW - 3:TW - 3 + n + 1] = 7
    image[TH - 2:TH - 2 + n, 5] = 9          # across the horizontal seam
    image[TH - 3:TH - 3 + n + 1, 11] = 9
    image[2 * TH - 1, TW + 20:TW + 20 + n - 1] = 4  # and one pixel in the tile below: an L of n
    image[2 * TH, TW + 20] = 4
    image[2 * TH - 1, 20:20 + n] = 4         # an L of n + 1
    image[2 * TH, 20] = 4
    r = images_of(Rig(hip_ctx, one(image)).check(n))[0]
    assert (r["n_removed"], r["n_kept"]) == (3 * n, 3 * (n + 1))


def test_lines_along_the_seams(hip_ctx):
    """one-pixel-wide lines on each side of a vertical and of a horizontal seam, apart in value so that they do not join each other"""
    image = np.zeros((2 * TH + 3, 2 * TW + 3), F)
    image[:, TW - 1], image[:, TW] = 1, 3
    image[TH - 1, :], image[TH, :] = 5, 7
    image[TH - 1:TH + 1, TW - 1:TW + 1] = [[9, 11], [13, 15]]  # the crossings belong to nobody
    rig = Rig(hip_ctx, one(image))
    r = images_of(rig.check(TH - 1))[0]
    assert r["n_removed"] == 4 + 2 * (TH - 1) and len(np.unique(r["label"])) == 13
    assert images_of(rig.check(TW - 1))[0]["n_removed"] == 4 + 2 * (TH - 1) + 2 * (TH + 2) + 2 * (TW - 1)
    # a max_diff of 2 joins each pair of lines across its seam, and the crossings two by two: six components
    r = images_of(rig.check(1, 2.0))[0]
    assert r["n_removed"] == 0 and len(np.unique(r["label"])) == 7


# ---- 3. long paths -------------------------------------------------------------------------------------------------------------------
def serpentine(rows, cols):
    """every other row whole, joined at alternating ends: one path from (0, 0) through every tile and across every seam many times"""
    m = np.zeros((rows, cols), bool)
    m[0::2, :] = True
    m[1::4, cols - 1] = True
    m[3::4, 0] = True
    return m


def spiral(rows, cols):
    """every other ring, each broken below its top left corner and joined to the next one inside it: one path from (0, 0) inwards"""
    m = np.zeros((rows, cols), bool)
    for k in range(0, min(rows, cols) // 2, 2):
        if rows - 2 * k < 1 or cols - 2 * k < 1:
            break
        m[k, k:cols - k] = m[rows - 1 - k, k:cols - k] = True
        m[k:rows - k, k] = m[k:rows - k, cols - 1 - k] = True
        if rows - 2 * k >= 5 and cols - 2 * k >= 5:
            m[k + 1, k] = False
            m[k + 2, k + 1] = True
    return m


def comb(rows, cols):
    """every other column whole, joined by the last row alone: every tooth is its own component until the spine is reached"""
    m = np.zeros((rows, cols), bool)
    m[:, 0::2] = True
    m[rows - 1, :] = True
    return m


PATHS = dict(serpentine=serpentine, serpentine_t=lambda r, c: serpentine(c, r).T, spiral=spiral, comb=comb, comb_t=lambda r, c: comb(c, r).T)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
@pytest.mark.parametrize("name", sorted(PATHS))
def test_long_paths(hip_ctx, name, dtype):
    rows, cols = 3 * TH, 3 * TW
    mask = PATHS[name](rows, cols)
    size = int(mask.sum())
    assert mask[0, 0] and size > rows * cols // 3
    rig = Rig(hip_ctx, one(mask.astype(dtype) * dtype(6)))
    for max_size, removed in ((size - 1, 0), (size, size)):
        r = images_of(rig.check(max_size, 0.0, name))[0]
        assert r["n_removed"] == removed and (r["label"][mask] == 0).all()  # the first pixel's index


# ---- 4. extremes of structure --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_one_component_singletons_and_nothing(hip_ctx, dtype):
    shape = (2 * TH + 3, 2 * TW + 5)
    n = shape[0] * shape[1]
    rig = Rig(hip_ctx, one(np.full(shape, 3, dtype)))
    for max_size, removed in ((0, 0), (1, 0), (200, 0), (n - 1, 0), (n, n), (2 ** 31 - 1, n)):
        r = images_of(rig.check(max_size))[0]
        assert r["n_removed"] == removed and not r["label"].any()
    board = (np.indices(shape).sum(axis=0) % 2 == 0)
    rig = Rig(hip_ctx, one(board.astype(dtype)))
    assert images_of(rig.check(0))[0]["n_removed"] == 0
    r = images_of(rig.check(1))[0]
    assert r["n_removed"] == board.sum() and r["n_kept"] == 0
    r = images_of(Rig(hip_ctx, one(np.zeros(shape, dtype))).check(5))[0]
    assert (r["n_removed"], r["n_kept"]) == (0, 0) and (r["label"] == -1).all()


# ---- 5. the comparison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1.0, 0.75, 1024.0])
def test_ramps_at_max_diff_and_one_ulp_above(hip_ctx, step):
    """k * step and the differences are exact; the ramps run along a row across a vertical seam and down a column across a horizontal
    one"""
    image = np.zeros((TH + 8, TW + 8), F)
    image[2, TW - 4:TW + 4] = np.arange(1, 9, dtype=F) * F(step)
    image[TH - 4:TH + 4, 9] = np.arange(1, 9, dtype=F) * F(step)
    rig = Rig(hip_ctx, one(image))
    r = images_of(rig.check(7, step))[0]
    assert r["n_removed"] == 0 and len(np.unique(r["label"])) == 3
    below = float(np.nextafter(F(step), F(0)))  # step is nextafter(below, inf)
    r = images_of(rig.check(7, below))[0]
    assert r["n_removed"] == 16 and len(np.unique(r["label"])) == 17


def test_a_chain_that_is_not_transitive(hip_ctx):
    image = np.zeros((TH + 2, TW + 2), F)
    image[1, TW - 2:TW + 1] = [1, 2, 3]      # the ends differ by 2: one component through the middle
    image[5, TW - 2:TW + 1] = [1, 3, 2]      # two
    image[TH - 1:TH + 1, 3:5] = [[1, 3], [2, 4]]  # two columns, joined down but not across
    r = images_of(Rig(hip_ctx, one(image)).check(2))[0]
    assert (r["n_removed"], r["n_kept"]) == (7, 3) and r["label"][1, TW] == TW + 2 + TW - 2


def test_values_that_are_not_numbers_or_not_positive(hip_ctx):
    rng = _rng(5)
    shape = (2, 1, TH + 3, TW + 7)
    images = noise(rng, shape, 0.8)
    for value in (NAN, INF, F(-1), F(-0.0), -INF, F(1e-45), F(3e38)):
        images[rng.random(shape) < 0.08] = value
    images[0, 0, 4, 10:14] = INF  # +inf beside +inf: valid and not connected
    images[0, 0, TH - 1:TH + 1, TW - 1:TW + 1] = INF
    rig = Rig(hip_ctx, images, np.where(np.isnan(images), F(4), images + F(1)))
    for max_size, max_diff in ((1, 1.0), (3, 0.0), (6, 3e38), (2 ** 31 - 1, 1.0)):
        results = rig.check(max_size, max_diff)
    assert images_of(results)[0]["label"][4, 11] == 4 * (TW + 7) + 11
    assert np.isnan(rig.outputs()["image"]).sum() == np.isnan(images).sum()  # the invalid pixels are not written


def test_the_extremes_of_16_bits(hip_ctx):
    image = noise(_rng(6), (TH + 1, TW + 9), 0.5, 2, np.uint16)
    image[image == 2] = 65535
    image[TH - 1:TH + 1, TW - 1:TW + 1] = [[65535, 1], [1, 65535]]
    rig = Rig(hip_ctx, one(image))
    a = images_of(rig.check(3, 65533))[0]
    b = images_of(rig.check(3, 65534))[0]  # 65535 - 1
    assert a["n_removed"] > b["n_removed"] > 0


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_max_diff_0_joins_equal_values_only(hip_ctx, dtype):
    images = noise(_rng(7), (2, 1, TH + 5, TW + 5), 0.9, 2, dtype)
    results = Rig(hip_ctx, images).check(6, 0.0)
    assert sum(i["n_removed"] for i in images_of(results)) > 100 and sum(i["n_kept"] for i in images_of(results)) > 100


# ---- 6. batches ----------------------------------------------------------------------------------------------------------------------
def batch_images(rng, B, frames, rows, cols, dtype=np.float32):
    """different content in every image; the last row of an image is the first row of the next one, valid throughout: a leak across
    images would join them"""
    images = noise(rng, (B, frames, rows, cols), 0.6, dtype=dtype)
    flat = images.reshape(B * frames, rows, cols)
    flat[:, 0, :] = 2
    flat[:, -1, :] = 2
    return images


def test_sequences_of_unequal_length(hip_ctx):
    images = batch_images(_rng(8), 3, 2, TH + 3, TW + 3)
    rig = Rig(hip_ctx, images, images + F(10), n_images=(2, 0, 1))
    for max_size in (3, TW + 3, 2 ** 31 - 1):
        results = rig.check(max_size)
        assert [r["status"] for r in results] == [0, 0, 0] and len(images_of(results)) == 3
    assert images_of(results)[0]["n_kept"] == 0
    Rig(hip_ctx, images).check(TW + 3)  # n_images not given: every image


def test_a_sequence_with_too_many_images_is_refused_alone(hip_ctx):
    images = batch_images(_rng(9), 2, 2, TH + 1, TW + 1, np.uint16)
    for n_images in ((3, 2), (1, -1)):
        results = Rig(hip_ctx, images, images.astype(F), n_images=n_images).check(TW + 1)
        assert [r["status"] for r in results] == [ref.PRS_ERR_RANGE if not 0 <= n <= 2 else 0 for n in n_images]


def test_the_flat_form(hip_ctx):
    images = batch_images(_rng(10), 3, 2, 9, TW + 2)
    rig = Rig(hip_ctx, images, images * F(2), n_images=(1, 2, 2), pad=2, flat=True)
    assert tuple(rig.inputs()["image"].shape) == (6, 9, TW + 2)
    rig.check(12)


# ---- 7. companion and outputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [(np.float32, np.float32), (np.uint16, None), (np.float32, np.uint16), (np.uint16, np.float32)])
def test_companions(hip_ctx, kinds):
    """the companion is not zero where the image is invalid, and stays so"""
    shape = (2, 2, TH + 2, TW + 6)
    images = noise(_rng(11), shape, 0.6, dtype=kinds[0])
    companions = None if kinds[1] is None else (_rng(11, 1).integers(1, 9, shape)).astype(kinds[1])
    rig = Rig(hip_ctx, images, companions, pad=1)
    results = rig.check(5)
    assert sum(i["n_removed"] for i in images_of(results)) > 50
    if companions is not None:
        left = rig.outputs()["companion"][..., :TW + 6]
        assert (left[images == 0] != 0).all() and (left == 0).sum() == sum(i["n_removed"] for i in images_of(results))


SUBSETS = [(), ("label",), ("n_kept",), ("n_removed",), ("label", "n_kept"), ("label", "n_removed"), ("n_kept", "n_removed"),
           ("label", "n_kept", "n_removed")]


@pytest.mark.parametrize("outputs", SUBSETS)
def test_optional_outputs(hip_ctx, outputs):
    images = noise(_rng(12), (2, 2, TH + 2, TW + 6), 0.6)
    rig = Rig(hip_ctx, images, outputs=outputs)
    assert sorted(rig.tensors()) == sorted(outputs + ("image", "status"))
    rig.check(5)


def test_default_outputs():
    assert ops.SpeckleFilterBatch(1, 1, 2, 2).label is None and ops.SpeckleFilterBatch(1, 1, 2, 2).n_removed is not None


# ---- 8. random fields ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.6, 0.7, 0.95])
def test_random_fields(hip_ctx, density, dtype):
    """three by two tiles, the last of each ragged; 0.6 is about the density at which the components of a square lattice become long
    and winding"""
    shape = (2, 2, 2 * TH - 3, 2 * TW + 9)
    rig = Rig(hip_ctx, noise(_rng(13, int(100 * density)), shape, density, 2, dtype), noise(_rng(13, 1), shape, 0.9, 7, np.float32), pad=3)
    removed = []
    for max_size, max_diff in ((0, 1.0), (1, 1.0), (5, 0.0), (50, 1.0), (200, 0.0), (2 ** 31 - 1, 1.0)):
        results = rig.check(max_size, max_diff)
        removed.append(sum(i["n_removed"] for i in images_of(results)))
    assert removed[0] == 0 and removed[1] <= removed[3] <= removed[5] and removed[5] > 0 and images_of(results)[0]["n_kept"] == 0


# ---- 9. determinism and capture ------------------------------------------------------------------------------------------------------
def test_two_runs_are_byte_identical(hip_ctx):
    images = noise(_rng(14), (3, 2, 3 * TH + 1, 2 * TW + 1), 0.6, 2)
    rig = Rig(hip_ctx, images, images + F(1))
    rig.check(30)
    first = rig.outputs()
    rig.check(30)
    rig.compare(rig.outputs(), first, "second run")


def test_captured_graph_replayed_on_new_images(hip_ctx):
    import torch
    ctx = hip_ctx
    shape = (3, 2, TH + 5, 2 * TW + 3)
    rig = Rig(ctx, noise(_rng(15), shape, 0.6), noise(_rng(15, 1), shape, 0.9, 5), n_images=(2, 0, 1))
    p, rp = ops.speckle_params(9, 1.0, **rig.types), ref.params(9, 1.0)
    inputs = rig.inputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.sf.run(ctx, p, **inputs)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.sf.run(ctx, p, **inputs)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    # other images and counts, a refused sequence among them
    for replay, counts in enumerate(((1, 2, 2), (0, 3, 2))):
        rig.upload(noise(_rng(15, 2, replay), shape, 0.5 + 0.2 * replay), noise(_rng(15, 3, replay), shape, 0.9, 5), counts)
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, results = rig.expected(rp)
        rig.compare(rig.outputs(), want, "replay %d" % replay)
        assert [r["status"] for r in results] == ([0, 0, 0] if replay == 0 else [0, ref.PRS_ERR_RANGE, 0])
        assert sum(i["n_removed"] for i in images_of(results)) > 0


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
def test_call_level_refusals_write_nothing(hip_ctx):
    shape = (2, 2, 9, 20)
    images = noise(_rng(16), shape, 0.6)
    rig = Rig(hip_ctx, images, images + F(1), n_images=(2, 2))
    lib, ctx = _lib.load(), hip_ctx._h
    P = lambda **kw: ops.speckle_params(**dict(dict(max_size=5, max_diff=1.0, pixel_type="f32"), **kw))  # noqa: E731
    D = lambda: rig.sf.descriptor(P(), **rig.inputs())  # noqa: E731

    def run(d, p=None):
        p = P() if p is None else p
        return lib.prs_speckle_batch_run(ctx, C.byref(p) if p != "null" else None, C.byref(d) if d is not None else None)

    rig.fill_sentinel()
    assert run(D()) == 0
    hip_ctx.synchronize()
    rig.upload(images, images + F(1), (2, 2))
    rig.fill_sentinel()
    assert run(None) == -1 and run(D(), "null") == -1
    for field in ("image", "status", "workspace"):
        d = D()
        setattr(d, field, None)
        assert run(d) == -1, field
    for field, value in (("batch", 0), ("frames", 0), ("rows", 0), ("cols", -1), ("pitch", 76), ("pitch", 82), ("companion_pitch", 76),
                         ("companion_pitch", 81), ("label_pitch", 76), ("label_pitch", 83)):
        d = D()
        setattr(d, field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("max_diff", -1.0), ("max_diff", float("nan")), ("max_diff", float("inf")), ("max_size", -1)):
        p = P()
        setattr(p, field, value)
        assert run(D(), p) == ref.PRS_ERR_RANGE, (field, value)
    for field, value in (("pixel_type", ops.PIXEL_U8), ("pixel_type", 3), ("pixel_type", -1), ("companion_type", ops.PIXEL_U8),
                         ("companion_type", 7)):
        p = P()
        setattr(p, field, value)
        assert run(D(), p) == -5, (field, value)
    for field, step in (("image", 2), ("companion", 1), ("workspace", 8), ("n_images", 2), ("label", 2), ("n_kept", 1), ("n_removed", 2),
                        ("status", 2)):
        d = D()
        setattr(d, field, getattr(d, field) + step)
        assert run(d) == -5, field
    # companion or label inside image, before its start but reaching into it, or at its last element
    nbytes = 2 * 2 * 9 * 80
    for field in ("companion", "label"):
        for at in (0, 4, -4, nbytes - 4):
            d = D()
            setattr(d, field, d.image + at)
            assert run(d) == -5, (field, at)
    # 2^16 x 2^15 pixels are too many for an image, 2^12 images of 2^10 x 2^10 too many for a call
    for rows, cols, frames in ((1 << 16, 1 << 15, 2), (1 << 10, 1 << 10, 1 << 12)):
        d = D()
        d.rows, d.cols, d.frames, d.pitch, d.companion_pitch, d.label_pitch = rows, cols, frames, 4 * cols, 4 * cols, 4 * cols
        d.companion, d.label = None, None  # so that no overlap is what refuses the call
        assert run(d) == -5, (rows, cols, frames)
    hip_ctx.synchronize()
    want, _ = rig.expected(ref.params(0))
    for k, v in rig.outputs().items():
        if k in ("image", "companion"):
            assert v.tobytes() == want[k].tobytes(), k
        else:
            assert (v.view(np.uint8) == SENTINEL).all(), k


def test_the_python_layer_refuses_what_it_cannot_describe(hip_ctx):
    import torch
    sf = ops.SpeckleFilterBatch(2, 2, 5, 6)
    p = ops.speckle_params()
    ok = torch.zeros((2, 2, 5, 6), dtype=torch.float32, device="cuda")
    for bad in (ok.to(torch.float64), ok[..., :5], ok[:, :, :4], ok.transpose(2, 3).contiguous().transpose(2, 3), ok[:, :1].expand(2, 2, 5, 6),
                torch.zeros((2, 2, 5, 6), dtype=torch.uint16, device="cuda")):
        with pytest.raises(ValueError):
            sf.descriptor(p, bad)
    with pytest.raises(ValueError):
        sf.descriptor(p, ok, ok.to(torch.float64))
    with pytest.raises(ValueError):
        sf.descriptor(p, ok, n_images=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.SpeckleFilterBatch(1, 1, 2, 2, outputs=("labels",))


# ---- 11. the chain -------------------------------------------------------------------------------------------------------------------
def pairs(rng, shape):
    """the noise pairs of the dense-stereo test: two unrelated images, where islands survive the uniqueness and the left-right test"""
    right = rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.integers(0, 256, shape, dtype=np.uint8), right


def test_dense_stereo_filter_dense_cloud(hip_ctx):
    """DenseStereoBatch on noise pairs, the filter in place on its disparity with its depth as the companion, DepthCloudBatch on that
    depth: disparity, depth and the cloud equal the same chain through the three restatements"""
    import torch

    import dense_stereo_ref as sref
    import depth_cloud_ref as dref
    cam = dict(fx=40.0, fy=40.0, cx=30.0, cy=8.0, baseline_m=0.5)
    kw = dict(n_disparities=16, min_disparity=0, aggregation_radius=1, uniqueness_percent=3, lr_max_diff=1)
    B, frames, rows, cols = 1, 2, TH + 5, TW + 6
    left, right = pairs(_rng(17), (B, frames, rows, cols))
    sp, fp = sref.params(20.0, **kw), ref.params(4, 1.0)
    stereo = sref.dense_stereo(left[0], right[0], None, sp)
    disparity = np.stack([i["disparity"] for i in stereo["results"]])
    depth = np.stack([i["depth"] for i in stereo["results"]])
    filtered = ref.speckle(disparity, depth, None, fp)
    removed = [i["n_removed"] for i in filtered["results"]]
    kept = [i["n_kept"] for i in filtered["results"]]
    assert min(removed) > 0 and min(kept) > 0  # the filter has something to remove and something to leave
    want_depth = np.stack([i["companion"] for i in filtered["results"]])
    assert ((want_depth > 0) == (np.stack([i["image"] for i in filtered["results"]]) > 0)).all()

    dev = torch.device("cuda", 0)
    ds = ops.DenseStereoBatch(B, frames, rows, cols)
    ds.run(hip_ctx, ops.dense_stereo_params(cam, **kw), torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    sf = ops.SpeckleFilterBatch(B, frames, rows, cols)
    sf.run(hip_ctx, ops.speckle_params(4, 1.0), ds.disparity, ds.depth)
    pose = np.zeros((frames, 4, 4), F)
    for i in range(frames):
        q, _ = np.linalg.qr(_rng(17, i).normal(size=(3, 3)))
        pose[i, :3, :3], pose[i, :3, 3], pose[i, 3, 3] = q * np.sign(np.linalg.det(q)), (i, -1.0, 0.5), 1
    pose = pose.reshape(1, frames, 16)
    dc = ops.DepthCloudBatch(B, frames, rows, cols, frames * rows * cols)
    ckw = dict(range_min=0.1, range_max=10.0, scale=1.0)
    n_images = torch.tensor([frames], dtype=torch.int32, device=dev)
    dc.run(hip_ctx, ops.depth_cloud_params(cam, depth_type="f32", **ckw), ds.depth, torch.from_numpy(pose).to(dev), n_images)
    hip_ctx.synchronize()
    assert sf.status.cpu().tolist() == [0] and sf.n_removed.cpu().tolist() == [removed] and sf.n_kept.cpu().tolist() == [kept]
    assert ds.disparity.cpu().numpy().tobytes() == np.stack([i["image"] for i in filtered["results"]])[None].tobytes()
    assert ds.depth.cpu().numpy().tobytes() == want_depth[None].tobytes()
    want = dref.depth_cloud(dict(depth=want_depth, n_images=frames, pose=pose[0]), dref.params(cam, **ckw), dc.out_stride)
    unfiltered = dref.depth_cloud(dict(depth=depth, n_images=frames, pose=pose[0]), dref.params(cam, **ckw), dc.out_stride)
    got = dc.cloud_of(0)
    n = want["n_out"]
    assert (got["status"], got["n_out"], got["n_total"]) == (0, n, want["n_total"]) and 0 < n < unfiltered["n_total"]
    assert got["xyz"].tobytes() == want["xyz"][:n].tobytes() and got["row"].tobytes() == want["pixel"][:n].tobytes()

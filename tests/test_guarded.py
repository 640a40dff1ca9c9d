"""The guard-band arena (tests/guarded.py) on the CPU: what it places, how it is aligned, how wide its bands are and what check()
reports."""
import pytest
import torch

import guarded
from guarded import Arena, MIN_BAND


def _arena(fill=0xFF):
    return Arena(fill, nbytes=4 << 20, device="cpu")


@pytest.mark.parametrize("fill", guarded.FILLS)
def test_a_fresh_arena_is_clean_and_planted_bytes_are_reported(fill):
    a = _arena(fill)
    a.take((7, 3), torch.float32, 4, "first")
    x = a.take((5, 4), torch.float32, 16, "xyz")
    a.take((9,), torch.int32, 4, "last")
    assert bytes(x.view(torch.uint8).flatten().tolist()) == bytes([fill]) * 80
    a.check()
    assert a.violations() == []
    rec = [r for r in a.arrays if r["name"] == "xyz"][0]
    other = fill ^ 0x5A
    a.buf[rec["start"] - 1] = other                       # one before
    a.buf[rec["start"] + rec["extent"]] = other           # one after
    a.buf[rec["before"]] = other                          # the far end of the leading band
    a.buf[rec["after"] - 1] = other                       # the far end of the trailing band
    band_before, band_after = rec["start"] - rec["before"], rec["after"] - rec["start"] - rec["extent"]
    assert a.violations() == [("xyz", "before", -band_before), ("xyz", "before", -1), ("xyz", "after", 0), ("xyz", "after", band_after - 1)]
    with pytest.raises(guarded.Violation, match=r"xyz before -1, xyz after \+0"):
        a.check()
    x.fill_(3.0)                                          # writing the array itself is no violation
    assert len(a.violations()) == 4


def test_an_understated_extent_moves_the_trailing_band_into_the_array():
    a = _arena()
    x = a.take((6,), torch.uint8, 1, "inlier", extent=5)
    a.check()
    x[4] = 1
    a.check()
    x[5] = 1                                              # the array's true last byte: behind the extent the harness was told
    assert a.violations() == [("inlier", "after", 0)]
    with pytest.raises(ValueError):
        a.take((6,), torch.uint8, 1, "longer", extent=7)  # never more than the memory


@pytest.mark.parametrize("align", [1, 2, 4, 8, 16])
def test_take_gives_exactly_the_alignment_asked_for(align):
    a = _arena()
    dtype = {1: torch.uint8, 2: torch.uint16, 4: torch.float32, 8: torch.float64, 16: torch.float32}[align]
    for n in (1, 3, 17, 1000, 4097):
        t = a.take((n,), dtype, align, "n%d" % n)
        assert t.data_ptr() % align == 0 and t.data_ptr() % (2 * align) != 0, (n, t.data_ptr())
        assert tuple(t.shape) == (n,) and t.dtype == dtype
    u = a.take((33, 65), torch.uint8, 1, "image")
    assert u.data_ptr() % 2 == 1
    with pytest.raises(ValueError):
        a.take((4,), torch.float32, 2)                    # below the element size
    a.check()


def test_a_band_is_a_whole_outermost_element_and_at_least_4096_bytes():
    a = _arena()
    a.take((3,), torch.int32, 4, "small")                               # 4096
    a.take((3, 301, 4), torch.float32, 16, "rows")                      # one sequence: 4816 bytes
    a.take((2, 2, 33, 68), torch.float32, 4, "images")                  # one sequence of two images: 17952 bytes
    a.take((2, 33, 65), torch.uint8, 1, "pitched", strides=(33 * 80, 80, 1))
    want = dict(small=MIN_BAND, rows=301 * 16, images=2 * 33 * 68 * 4, pitched=MIN_BAND)
    end = 0
    for r in a.arrays:
        before, after = r["start"] - r["before"], r["after"] - r["start"] - r["extent"]
        assert before >= want[r["name"]] and after >= want[r["name"]], r
        assert r["before"] >= end                                        # bands are not shared between arrays
        end = r["after"]
    assert end < a.nbytes                                                # nothing adjoins the end of the allocation
    pitched = [r for r in a.arrays if r["name"] == "pitched"][0]
    assert pitched["extent"] == (2 * 33 - 1) * 80 + 65                   # to the last pixel of the last row
    with pytest.raises(MemoryError):
        a.take((a.nbytes,), torch.uint8, 1)


def test_adopt_keeps_values_shape_and_strides():
    class Holder:
        pass

    h = Holder()
    h.plain = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    storage = torch.arange(2 * 5 * 8, dtype=torch.int32).reshape(2, 5, 8)
    h.view = storage[..., :6]                                            # a pitch above cols
    h.u16 = torch.arange(10, dtype=torch.int32).to(torch.uint16)
    d = dict(depth=torch.arange(12, dtype=torch.float64).reshape(3, 4))
    a = _arena(0x00)
    before = {k: getattr(h, k).clone() for k in ("plain", "view", "u16")}
    for k, align in (("plain", 16), ("view", 4), ("u16", 2)):
        new = a.adopt(h, k, align)
        assert new is getattr(h, k) and a.base <= new.data_ptr() < a.base + a.nbytes
        assert new.shape == before[k].shape and new.dtype == before[k].dtype and torch.equal(new.to(torch.int64), before[k].to(torch.int64))
        assert new.data_ptr() % align == 0 and new.data_ptr() % (2 * align) != 0
    assert h.view.stride() == (40, 8, 1) and h.plain.stride() == (12, 4, 1)
    a.adopt(d, "depth", 8)
    assert torch.equal(d["depth"], torch.arange(12, dtype=torch.float64).reshape(3, 4)) and d["depth"].data_ptr() % 16 == 8
    a.check()
    # paint: slack inside an array becomes the fill, the rest stays
    b = _arena(0xFF)
    v = b.adopt(dict(x=storage[..., :6].clone(memory_format=torch.preserve_format)), "x", 4)
    b.paint(v[1, 3:])
    assert (v[1, 3:] == -1).all() and torch.equal(v[0], storage[0, :, :6]) and torch.equal(v[1, :3], storage[1, :3, :6])
    b.check()


def test_same_bytes_allows_untouched_fill_only():
    import numpy as np
    a = dict(x=np.array([1.5, 0.0, 2.5], np.float32), n=np.array([3, 0], np.int32))
    b = dict(x=np.array([1.5, np.nan, 2.5], np.float32), n=np.array([3, -1], np.int32))
    b["x"].view(np.uint32)[1] = 0xFFFFFFFF
    guarded.same_bytes(a, b)                              # slack holds each run's fill
    b["x"][2] = 2.75
    with pytest.raises(AssertionError, match="x differs"):
        guarded.same_bytes(a, b)
    with pytest.raises(AssertionError):
        guarded.same_bytes(b, dict(a, x=b["x"]))          # the 0xFF run's fill in the 0x00 run's place


def test_adopt_all_moves_shared_tensors_once_and_rebuilds_views():
    class Batch:
        pass

    maps, sess = Batch(), Batch()
    maps.coords = torch.arange(2 * 5 * 4, dtype=torch.float32).reshape(2, 5, 4)
    maps.n_corr = torch.zeros(2, dtype=torch.int32)
    maps._label = torch.arange(2 * 3 * 8, dtype=torch.int32).reshape(2, 3, 8)
    maps.label = maps._label[..., :5]
    maps.name = "not a tensor"
    a = _arena()
    a.adopt_all(dict(maps=maps))
    assert a.owns(maps.coords) and maps.coords.data_ptr() % 32 == 16 and maps.n_corr.data_ptr() % 8 == 4
    assert maps.label.data_ptr() == maps._label.data_ptr() and maps.label.stride() == (24, 8, 1) and maps.label[1, 2, 4] == 44
    sess.n_corr_merge = torch.tensor([7, 9], dtype=torch.int32)
    maps.n_corr = sess.n_corr_merge                        # what ops.SessionBatch does to its maps
    a.adopt_all(dict(sess=sess))
    assert maps.n_corr is sess.n_corr_merge and a.owns(maps.n_corr) and maps.n_corr.tolist() == [7, 9]
    assert [r["name"] for r in a.arrays] == ["maps._label", "maps.coords", "maps.n_corr", "sess.n_corr_merge"]
    a.adopt_all(dict(maps=maps, sess=sess))                # nothing moves twice
    assert len(a.arrays) == 4
    a.check()

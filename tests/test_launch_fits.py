"""The launch-size rule the launchers share (prs_launch_fits, prs::grid_fits in csrc/prs_host.h): HIP takes no launch of 2^32 or more
work-items in a grid dimension, so the ceiling is 2^24 - 1 workgroups of 256 threads, not the 2^31 - 1 workgroups a grid's type
would hold.  A pure function of the C-ABI.  No GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def fits():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "prs_launch_fits") and "prs_launch_fits" in _lib.SYMBOLS
    return _lib.load().prs_launch_fits


@pytest.mark.parametrize("limit,threads", [(1 << 24, 256), (1 << 23, 512), (1 << 22, 1024), (1 << 26, 64), (1 << 32, 1)])
def test_the_last_grid_that_fits_and_the_first_that_does_not(fits, limit, threads):
    assert fits(limit - 1, threads) == 1 and (limit - 1) * threads <= 0xffffffff
    assert fits(limit, threads) == 0 and limit * threads > 0xffffffff
    assert fits(1, threads) == 1


def test_threads_that_do_not_divide_2_to_the_32(fits):
    for threads in (192, 320, 1000):
        last = 0xffffffff // threads
        assert fits(last, threads) == 1 and fits(last + 1, threads) == 0, threads


@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_nothing_and_less_do_not_fit(fits, threads):
    for workgroups in (0, -1, -(1 << 24), -(1 << 62), -(1 << 63)):
        assert fits(workgroups, threads) == 0, workgroups


@pytest.mark.parametrize("threads", [1, 64, 256, 1024])
def test_counts_whose_product_would_overflow(fits, threads):
    """2^62 * 256 is 0 in 64 bits and 2^54 * 1024 is negative: neither may be read as a small grid"""
    for workgroups in (1 << 32, 1 << 54, 1 << 56, 1 << 62, (1 << 63) - 1):
        assert fits(workgroups, threads) == 0, workgroups


def test_a_workgroup_has_1_to_1024_threads(fits):
    for threads in (0, -1, -256, 1025, 1 << 20, -(1 << 31)):
        assert fits(1, threads) == 0, threads

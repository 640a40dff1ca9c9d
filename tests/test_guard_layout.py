"""The layout rule of the library's own allocations (prs_guard_layout, prs::guard_layout in csrc/prs_host.h): pure, no context, no
device.  Every device or pinned block of the library is sized by it.  With guard mode off it has to give the bytes each site has
always requested -- the request itself (a prs_map, a prs_pcf block, a place database or bank), the request plus a quarter plus 4096
(the work arenas, the small staging arenas, the aligner's job buffers) or plus a half plus 4096 (the default staging arena and the
pinned arena) -- so the default path allocates what it always did.  With guard mode on the user bytes lie behind a front band of
guarded.MIN_BAND bytes and the tail band begins at the first byte behind the request, never smaller than the slack it replaces."""
import ctypes as C

import pytest

import guarded
from srrg2_proslam_amd import _lib

SIZES = (0, 1, 4095, 4096, 4097, 3 * (1 << 20) + 17)
# what each rule adds to a request with guard mode off, restated from the sites as they were before they shared one path
SLACK = {
    _lib.GUARD_SLACK_EXACT: lambda n: 0,
    _lib.GUARD_SLACK_QUARTER: lambda n: n // 4 + 4096,
    _lib.GUARD_SLACK_HALF: lambda n: n // 2 + 4096,
}


def layout(nbytes, rule, guard):
    out = _lib.GuardExtent()
    assert _lib.load().prs_guard_layout(nbytes, rule, guard, C.byref(out)) == _lib.OK
    return out.total, out.user_offset, out.tail_bytes


def test_the_band_is_the_harness_band_and_the_pattern_is_neither_fill():
    assert _lib.GUARD_BAND == guarded.MIN_BAND == 4096
    assert _lib.GUARD_PATTERN not in guarded.FILLS and 0 < _lib.GUARD_PATTERN < 256


@pytest.mark.parametrize("rule", sorted(SLACK))
@pytest.mark.parametrize("nbytes", SIZES)
def test_guard_off_requests_what_the_site_always_requested(rule, nbytes):
    total, offset, tail = layout(nbytes, rule, 0)
    assert total == nbytes + SLACK[rule](nbytes)
    assert offset == 0 and tail == total - nbytes


@pytest.mark.parametrize("rule", sorted(SLACK))
@pytest.mark.parametrize("nbytes", SIZES)
def test_guard_on_tail_begins_at_the_request_and_covers_the_slack(rule, nbytes):
    total, offset, tail = layout(nbytes, rule, 1)
    assert offset == guarded.MIN_BAND  # the user pointer keeps the allocator's alignment
    assert tail == max(guarded.MIN_BAND, SLACK[rule](nbytes))  # never smaller than the slack: no silent overrun can become a fault
    assert total == offset + nbytes + tail  # the tail band begins at the first byte behind the request: no rounding, no slack
    assert total >= layout(nbytes, rule, 0)[0] + offset


def test_unknown_rule_and_missing_result_are_refused():
    out = _lib.GuardExtent()
    lib = _lib.load()
    assert lib.prs_guard_layout(16, 3, 0, C.byref(out)) == _lib.ERR_UNSUPPORTED
    assert lib.prs_guard_layout(16, -1, 1, C.byref(out)) == _lib.ERR_UNSUPPORTED
    assert lib.prs_guard_layout(16, 0, 0, None) == _lib.ERR_NULL

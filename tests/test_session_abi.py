"""The local-map manager's C-ABI: exported entries, struct sizes and key offsets, and the unchanged version."""
import ctypes as C

from srrg2_proslam_amd import _lib


def test_entries_are_exported_and_the_version_stays():
    lib = _lib.load()
    for name in ("prs_session_step_batch", "prs_session_unroll_batch", "prs_session_struct_sizes"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.prs_version() == 104 == _lib.ABI_VERSION


def test_struct_sizes_and_offsets():
    sizes = (C.c_uint64 * 2)()
    _lib.load().prs_session_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.SessionParams), C.sizeof(_lib.SessionBatch)]
    assert C.sizeof(_lib.SessionParams) == 16
    # six int32, then 34 pointers: the first at byte 24, the last at 24 + 33 * 8
    b = _lib.SessionBatch
    assert C.sizeof(b) == 24 + 34 * 8
    assert (b.batch.offset, b.handover_stride.offset, b.pose.offset) == (0, 20, 24)
    assert (b.X.offset, b.coords.offset, b.graph_X.offset) == (24 + 10 * 8, 24 + 13 * 8, 24 + 21 * 8)
    assert (b.handover_desc.offset, b.graph_id_base.offset) == (24 + 29 * 8, 24 + 33 * 8)

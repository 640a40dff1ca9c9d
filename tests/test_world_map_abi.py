"""The world map's part of the C-ABI: the workspace size, the null-context refusal and the params helper (the layouts are
tests/test_abi_layout.py).  No GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_workspace_bytes(built):
    lib = built.load()
    f = lib.prs_world_map_workspace_bytes
    # per (sequence, map entry, chunk of 256 rows) two counts and six bounds of 4 bytes, per (sequence, map entry) a node; the map
    # entries are the slots and the live map; rounded up to 16 bytes
    assert f(1, 1, 1) == 80 and f(1, 1, 256) == 80 and f(1, 1, 257) == 144
    assert f(3, 5, 4096) == (4 * 3 * 6 * (16 * 8 + 1) + 15) // 16 * 16
    assert f(4096, 4, 4096) % 16 == 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert f(*bad) == 0


def test_null_context_is_refused(built):
    p, o = built.WorldMapParams(), built.WorldMapBatch()
    s, m, a = built.SessionBatch(), built.MergeBatch(), built.MapArchive()
    rc = built.load().prs_world_map_batch_run(None, C.byref(p), C.byref(s), C.byref(m), C.byref(a), C.byref(o))
    assert rc == -1  # PRS_ERR_NULL


def test_params_helper(built):
    from srrg2_proslam_amd import ops
    p = ops.world_map_params()
    assert (p.min_n_opt, p.require_inlier, p.include_live, p.refresh_state) == (0, 0, 1, 0)
    q = ops.world_map_params(min_n_opt=3, require_inlier=True, include_live=False, refresh_state=True)
    assert (q.min_n_opt, q.require_inlier, q.include_live, q.refresh_state) == (3, 1, 0, 1)
    with pytest.raises(ValueError):
        ops.world_map_params(min_n_opt=-1)

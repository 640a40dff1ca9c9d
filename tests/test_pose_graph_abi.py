"""The pose-graph optimiser's own status code and its workspace size (the layouts are tests/test_abi_layout.py; no GPU needed)."""
import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import _lib
    return _lib


def test_not_positive_definite_has_its_own_status_string(built):
    assert built.load().prs_status_string(built.ERR_NOT_POSITIVE_DEFINITE) != built.load().prs_status_string(-99)


def test_workspace_bytes(built):
    f = built.load().prs_pose_graph_workspace_bytes
    assert f(1, 114, 1064) == 1064 * 288 and f(64, 455, 21967) == 64 * 21967 * 288 and f(0, 8, 8) == 0

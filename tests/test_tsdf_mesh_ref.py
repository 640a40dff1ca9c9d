"""Properties of the TSDF mesh's restatement (tests/tsdf_mesh_ref.py) on volumes whose mesh is known: an analytic sphere (closed,
oriented, Euler characteristic 2, the sphere's radius and volume), a tilted plane through the whole grid at several sizes (a disc:
Euler characteristic 1), the fused sphere scene of the fusion's tests (open), a random volume with values that are not distances
(the non-manifold case), and the two strides.  The expected counts were worked out with a prototype of the rule.  No GPU needed."""
import numpy as np
import pytest

import tsdf_mesh_ref as ref
import tsdf_mesh_rig as rig
import tsdf_ref
from tsdf_rig import sentinel

F = np.float32
P = rig.host_params()


def whole(volume, origin, p=P):
    """the mesh with strides that hold all of it, and the crossings it came from"""
    voxels = volume.shape[0] * volume.shape[1] * volume.shape[2]
    m = ref.mesh(volume, p, origin, voxels, 3 * voxels)
    assert m["status"] == tsdf_ref.PRS_OK
    cell, _, _ = ref.crossings(volume, p, origin)
    return m, cell


def topology(m):
    """(V, E, F, boundary edges, the most quads on an edge, the most quads on a directed edge, vertices a quad names)"""
    quad = m["quad"][:m["n_quads"]]
    undirected, directed = ref.edge_use(quad)
    uses = list(undirected.values())
    return (m["n_vertices"], len(undirected), len(quad), sum(1 for u in uses if u == 1), max(uses, default=0),
            max(directed.values(), default=0), len(np.unique(quad)))


def test_analytic_sphere_is_closed_oriented_and_round():
    volume, origin = rig.sphere_volume()
    m, cell = whole(volume, origin)
    assert (len(cell), m["n_vertices"], m["n_quads"]) == (362, 364, 362)   # all crossings interior
    V, E, Fc, boundary, most, most_directed, used = topology(m)
    undirected, directed = ref.edge_use(m["quad"][:Fc])
    assert set(undirected.values()) == {2} and set(directed.values()) == {1}
    assert V - E + Fc == 2 and boundary == 0 and used == V
    xyz = m["vertex"][:V, :3].astype(np.float64)
    radius = np.linalg.norm(xyz - rig.SPHERE_CENTRE, axis=1)
    print("radius %.4f .. %.4f" % (radius.min(), radius.max()))
    assert np.abs(radius - rig.SPHERE_RADIUS).max() <= rig.VS / 4
    tri = xyz[ref.triangles(m["quad"][:Fc])]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", normal, tri.mean(1) - rig.SPHERE_CENTRE) > 0).all()   # away from the centre
    signed = np.einsum("ij,ij->i", tri[:, 0] - rig.SPHERE_CENTRE, np.cross(tri[:, 1] - rig.SPHERE_CENTRE, tri[:, 2] - rig.SPHERE_CENTRE)).sum() / 6
    exact = 4 / 3 * np.pi * rig.SPHERE_RADIUS ** 3
    print("volume %.4f against %.4f" % (signed, exact))
    assert abs(signed - exact) <= 0.1 * exact
    # the vertex normals point outwards too, and the fourth floats are what the header says
    n = m["normal"][:V]
    assert (n[:, 3] == 1).all() and (np.einsum("ij,ij->i", n[:, :3].astype(np.float64), xyz - rig.SPHERE_CENTRE) > 0).all()
    assert m["vertex"][:V, 3].min() >= 1 and m["vertex"][:V, 3].max() <= 12 and m["vertex"][:V, 3].sum() == 4 * 362


def test_tilted_plane_is_a_disc():
    volume, origin = rig.plane_volume((9, 7, 6))
    m, cell = whole(volume, origin)
    assert (len(cell), m["n_quads"], m["n_vertices"]) == (94, 58, 75)
    V, E, Fc, boundary, most, most_directed, used = topology(m)
    assert (boundary, most, most_directed) == (32, 2, 1)
    assert used - E + Fc == 1   # over the vertices the quads use: the cubes of boundary crossings hold vertices no quad names


@pytest.mark.parametrize("dims, vertices, used, quads", [((2, 2, 2), 1, 0, 0), ((1, 5, 5), 0, 0, 0), ((2, 9, 3), 11, 6, 2),
                                                        ((70, 9, 6), 184, 184, 153), ((33, 5, 9), 144, 142, 107)])
def test_tilted_plane_at_other_sizes(dims, vertices, used, quads):
    volume, origin = rig.plane_volume(dims)
    m, cell = whole(volume, origin)
    assert (m["n_vertices"], m["n_quads"], len(np.unique(m["quad"][:m["n_quads"]]))) == (vertices, quads, used)
    if dims == (70, 9, 6):
        assert len(cell) == 217
    if dims[0] == 1:
        assert len(cell) > 0   # crossings, but no cube to hold a vertex
    V, E, Fc, boundary, most, most_directed, _ = topology(m)
    assert most <= 2 and most_directed <= 1 and (quads == 0 or used - E + Fc == 1)


def test_fused_sphere_scene_is_an_open_mesh():
    volume, origin = rig.fused_sphere()
    m, cell = whole(volume, origin)
    assert (len(cell), m["n_vertices"], m["n_quads"]) == (898, 1007, 898)
    V, E, Fc, boundary, most, most_directed, used = topology(m)
    assert (boundary, most, most_directed) == (230, 2, 1)


def test_random_volume_with_values_that_are_no_distances():
    volume, origin = rig.random_volume()
    assert np.isnan(volume[..., 0]).any() and np.isposinf(volume[..., 0]).any() and np.isneginf(volume[..., 0]).any()
    m, cell = whole(volume, origin)
    nv, nq = m["n_vertices_total"], m["n_quads_total"]
    assert nv > 0 and nq > 0 and m["quad"][:nq].min() >= 0 and m["quad"][:nq].max() < nv
    assert (np.diff(m["cube"][:nv]) > 0).all()
    edge = m["edge"][:nq]
    assert (np.diff(edge) > 0).all() and np.isin(edge, cell).all() and nq < len(cell)
    assert np.isfinite(m["vertex"][:nv]).all()
    undirected, _ = ref.edge_use(m["quad"][:nq])
    assert 4 in set(undirected.values())   # the non-manifold case
    assert (m["normal"][:nv, 3] == 0).any() and (m["normal"][:nv, 3] == 1).any()


def test_min_weight_above_every_weight_gives_nothing():
    volume, origin = rig.random_volume()
    m = ref.mesh(volume, rig.host_params(min_weight=3.0), origin, 8, 8)
    assert (m["status"], m["n_vertices_total"], m["n_quads_total"]) == (tsdf_ref.PRS_OK, 0, 0)


def test_strides_exactly_full_and_one_short():
    volume, origin = rig.plane_volume((9, 7, 6))
    full, _ = whole(volume, origin)
    nv, nq = full["n_vertices_total"], full["n_quads_total"]
    for vcap, qcap in ((nv, nq), (nv - 1, nq), (nv, nq - 1), (3, 2)):
        before = dict(vertex=sentinel((vcap, 4), F), normal=sentinel((vcap, 4), F), quad=sentinel((qcap, 4), np.int32),
                      cube=sentinel((vcap,), np.int32), edge=sentinel((qcap,), np.int32))
        m = ref.mesh(volume, P, origin, vcap, qcap, before)
        over = vcap < nv or qcap < nq
        assert m["status"] == (tsdf_ref.PRS_ERR_CAPACITY if over else tsdf_ref.PRS_OK)
        assert (m["n_vertices"], m["n_vertices_total"], m["n_quads"], m["n_quads_total"]) == (min(nv, vcap), nv, min(nq, qcap), nq)
        for name in ("vertex", "normal", "cube"):
            assert m[name].tobytes() == full[name][:vcap].tobytes(), name      # a prefix of the whole mesh: ranks do not move
        for name in ("quad", "edge"):
            assert m[name].tobytes() == full[name][:qcap].tobytes(), name
    # a longer array keeps what lies behind the counts
    before = dict(vertex=sentinel((nv + 2, 4), F), normal=sentinel((nv + 2, 4), F), quad=sentinel((nq + 3, 4), np.int32),
                  cube=sentinel((nv + 2,), np.int32), edge=sentinel((nq + 3,), np.int32))
    m = ref.mesh(volume, P, origin, nv + 2, nq + 3, before)
    for name, n in (("vertex", nv), ("normal", nv), ("cube", nv), ("quad", nq), ("edge", nq)):
        assert m[name][n:].tobytes() == before[name][n:].tobytes() and m[name][:n].tobytes() == full[name][:n].tobytes(), name
    # count only: the totals, nothing else
    m = ref.mesh(volume, P, origin, nv + 2, nq + 3, before, count_only=True)
    assert (m["status"], m["n_vertices"], m["n_vertices_total"], m["n_quads"], m["n_quads_total"]) == (tsdf_ref.PRS_OK, 0, nv, 0, nq)
    for name in before:
        assert m[name].tobytes() == before[name].tobytes(), name

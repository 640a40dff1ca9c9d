"""Seeded inputs shared by the world voxel filter's tests (tests/world_voxel_ref.py is the restatement they are compared with).  A cloud
is one sequence in the layout world_voxel_ref.world_voxel takes; every row of every array is filled, rows from n on too, so that a
kernel reading past n shows."""
import numpy as np

F = np.float32
SIDE = 100  # voxels per axis the seeded clouds spread over, centred on the origin


def cells_of(rng, n_voxels, side=SIDE):
    """n_voxels distinct voxel indices [n_voxels, 3] in [-side / 2, side / 2)"""
    flat = rng.choice(side ** 3, size=n_voxels, replace=False)
    return np.stack([flat // side ** 2, flat // side % side, flat % side], axis=1).astype(np.int64) - side // 2


def make_cloud(rng, in_stride, n, voxel_size, n_voxels, max_n_opt=6, side=SIDE):
    """rows spread at random over n_voxels distinct voxels (so the rows of one voxel interleave with those of the others); when
    n >= n_voxels the first n_voxels rows take one voxel each in a random order, so rows 0 .. n - 1 hold exactly n_voxels voxels.
    Coordinates keep 5 % of a voxel away from its faces: float32 rounding cannot move a row out.  node and row ascend as a world map's
    do (node-then-row order).  side: the voxels per axis, for a cloud of more than SIDE ** 3 voxels"""
    N = int(in_stride)
    cells = cells_of(rng, max(int(n_voxels), 1), side)
    pick = rng.integers(0, cells.shape[0], N)
    lead = min(N, cells.shape[0])
    pick[:lead] = rng.permutation(cells.shape[0])[:lead]
    xyz = np.empty((N, 4), F)
    xyz[:, :3] = ((cells[pick] + rng.uniform(0.05, 0.95, (N, 3))) * np.float64(F(voxel_size))).astype(F)
    xyz[:, 3] = rng.normal(size=N).astype(F)
    i = np.arange(N)
    return dict(in_stride=N, n=int(n), xyz=xyz, n_opt=rng.integers(0, max_n_opt, N).astype(np.uint32),
                desc=rng.integers(0, 256, (N, 32), dtype=np.uint8), node=(i // 37).astype(np.int32), row=(i % 37).astype(np.int32))


def one_voxel_cloud(rng, in_stride, n, voxel_size, cell=(-3, 0, 7)):
    """every row in the one voxel `cell`: the worst contention on a slot"""
    c = make_cloud(rng, in_stride, n, voxel_size, 1)
    c["xyz"][:, :3] = ((np.asarray(cell) + rng.uniform(0.05, 0.95, (int(in_stride), 3))) * np.float64(F(voxel_size))).astype(F)
    return c


HIGHEST_N_OPT = np.uint32(0xFFFFFFFF)


def plant_chunk_counts(cloud, n_voxels, full, empty):
    """chunks of 256 rows with a known number of representatives, in a cloud of make_cloud whose first n_voxels rows take one voxel
    each.  Every row of the chunks `full` (inside those first rows) gets the highest n_opt, so each represents its voxel: a count of
    256.  The chunks `empty` (behind those first rows) repeat the coordinates of rows 0 .. 255 with n_opt 0: rows 0 .. 255 hold the
    same voxels at a lower index and win every tie, so none of the chunk's rows represents: a count of 0.  No voxel is added or lost"""
    for c in full:
        assert 256 * (c + 1) <= n_voxels
        cloud["n_opt"][256 * c: 256 * (c + 1)] = HIGHEST_N_OPT
    for c in empty:
        assert 256 * c >= n_voxels and 256 * (c + 1) <= cloud["n"]
        cloud["xyz"][256 * c: 256 * (c + 1), :3] = cloud["xyz"][:256, :3]
        cloud["n_opt"][256 * c: 256 * (c + 1)] = 0


def chunk_counts(index, chunks):
    """the input rows of the representatives (a result's `index`, not truncated) -> (representatives per chunk of 256 rows [chunks], the
    first output row of every chunk [chunks])"""
    counts = np.bincount(np.asarray(index, np.int64) // 256, minlength=chunks)
    return counts, np.cumsum(counts) - counts


def spread_n_opt(rng, cloud, voxel_size, values):
    """n_opt drawn from `values` (ascending) so that voxels differ in the highest value they hold: the rows of voxel v draw from the
    first 1 + v % len(values) values"""
    from world_voxel_ref import voxel_index, voxel_key
    k = voxel_index(cloud["xyz"][:, :3], np.float64(F(voxel_size))).astype(np.int64)
    _, inv = np.unique(voxel_key(k), return_inverse=True)
    values = np.asarray(values, np.uint32)
    cloud["n_opt"] = values[rng.integers(0, 1 + inv.reshape(-1) % len(values))]


# coordinates with a known fate at voxel size 0.5 (exact in float32, so is every multiple): (value, voxel index or the drop's name)
EDGE_SIZE = F(0.5)
EDGES = [
    (F(-1e-30), -1),                # floor, not truncation
    (F(-0.0), 0),
    (F(-0.25), -1),
    (F(-1.5), -3),                  # exactly on a face: belongs to the voxel above it
    (F(2.0), 4),
    (F(524287.75), (1 << 20) - 1),  # the last voxel inside
    (F(524288.0), "outside"),       # the first outside
    (F(-524288.0), -(1 << 20)),     # the first voxel inside
    (np.nextafter(F(-524288.0), F(-np.inf)), "outside"),
    (F(np.nan), "nonfinite"),
    (F(np.inf), "nonfinite"),
    (F(-np.inf), "nonfinite"),
    (F(3e38), "outside"),
]


def plant_edges(cloud, rows):
    """writes the EDGES, cycling, into coordinate (row % 3) of the given rows of a cloud built for EDGE_SIZE; -> [(row, axis, fate)]"""
    planted = []
    for j, r in enumerate(rows):
        value, fate = EDGES[j % len(EDGES)]
        cloud["xyz"][r, r % 3] = value
        planted.append((int(r), int(r % 3), fate))
    return planted

"""ops.DenseTrackerBatch restated: the restatements of its four stages chained as start() and step() chain the device calls --
tests/tsdf_ref.py's integrate of one image, tests/tsdf_raycast_ref.py's raycast of one view at pose k - 1 with a step of one voxel,
tests/dense_align_ref.py's schedule from the identity without live normals, the two pose_compose_batch calls as the checker's
se3_mul and se3_inverse (oracle/, which tests/test_pose_algebra_gpu.py shows equal to the kernel bit for bit), and the integrate
at pose k.  No arithmetic of its own: every float32 operation is one a device test already pins byte for byte.  `compose` swaps
the composition for a wrong one, which tests/test_dense_loop_ref.py shows the scene tells apart.  Test infrastructure only."""
import functools
import hashlib

import numpy as np

import dense_align_ref
import dense_loop_cases as cases
import tsdf_mesh_ref
import tsdf_raycast_ref
import tsdf_ref
from srrg2_proslam_amd import configs

F = np.float32
EYE = np.eye(4, dtype=F)
MESH_STRIDE = 60000


def compose_tracker(pose, X):
    """pose k = pose k - 1 * X as DenseTrackerBatch.step makes it of two calls of pose_compose_batch(P, X) = P * X^-1"""
    from oracle import binding as ob
    inverse = ob.se3_mul(EYE, ob.se3_inverse(X))
    return ob.se3_mul(pose, ob.se3_inverse(inverse))


def compose_left(pose, X):
    """X * pose: the wrong side"""
    from oracle import binding as ob
    return ob.se3_mul(X, pose)


def compose_inverted(pose, X):
    """pose * X^-1: pose_compose_batch called once, as its name suggests"""
    from oracle import binding as ob
    return ob.se3_mul(pose, ob.se3_inverse(X))


def compose_kept(pose, X):
    """X ignored"""
    return np.array(pose, F)


MUTANTS = {"X * pose": compose_left, "pose * X^-1": compose_inverted, "pose kept": compose_kept}


def settings(depth_type, camera=cases.CAMERA, voxel_size=cases.VS, truncation=cases.TRUNCATION):
    """(tsdf, raycast, align) parameters of the three restatements, as DenseTrackerBatch derives its three from one camera"""
    scale = cases.SCALE[depth_type]
    return (tsdf_ref.params(camera, voxel_size=voxel_size, truncation=truncation, scale=scale),
            tsdf_raycast_ref.params(camera, voxel_size=voxel_size, step=voxel_size),
            dense_align_ref.params(camera, depth_type, scale))


def digest(volume):
    return hashlib.sha256(np.ascontiguousarray(volume, F).tobytes()).hexdigest()


def track(frames, pose0, depth_type, origin, dims, schedule, compose=None, **kw):
    """frames [n, rows, cols] of depth_type, pose0 [4, 4]: the pose of frame 0; dims = (nx, ny, nz); kw: settings()'s
    -> (steps, volume): steps[k] for k = 0 .. n - 1 is dict(pose [4, 4] float32, X, result, mask, n_updates, volume: the sha256 of
    the volume after frame k was fused) with X, result and mask (the aligner's, of the schedule's last call) None at k = 0;
    volume [nz, ny, nx, 2] float32 after the last frame"""
    compose = compose_tracker if compose is None else compose
    fp, rp, ap = settings(depth_type, **kw)
    frames = np.asarray(frames)
    n, rows, cols = frames.shape
    nx, ny, nz = dims
    volume = np.zeros((nz, ny, nx, 2), F)
    pose = np.tile(EYE.reshape(16), (n, 1))
    pose[0] = np.asarray(pose0, F).reshape(16)

    def fuse(k):
        out = tsdf_ref.integrate(dict(depth=frames[k][None], pose=pose, frame_index=[k]), fp, origin, volume)
        assert out["status"] == 0 and out["n_skipped"] == 0
        return out["volume"], int(out["n_updates"][0])

    volume, updates = fuse(0)
    steps = [dict(pose=pose[0].reshape(4, 4).copy(), X=None, result=None, mask=None, n_updates=updates, volume=digest(volume))]
    for k in range(1, n):
        model = tsdf_raycast_ref.raycast(dict(pose=pose, view_index=[k - 1]), rp, origin, volume, 1, rows, cols)
        assert model["status"] == 0 and model["n_skipped"] == 0
        X, result, mask = dense_align_ref.align_schedule(ap, EYE, model["depth"][0], model["normal"][0], frames[k], None, schedule)
        pose[k] = compose(pose[k - 1].reshape(4, 4), X).reshape(16)
        volume, updates = fuse(k)
        steps.append(dict(pose=pose[k].reshape(4, 4).copy(), X=X, result=result, mask=mask, n_updates=updates, volume=digest(volume),
                          n_hit=int(model["n_hit"][0])))
    return steps, volume


# ---- the runs the tests share, made once a process ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tracked(name, depth_type, mutant=None, n_frames=cases.FRAMES):
    """track() on the first n_frames of a trajectory of tests/dense_loop_cases.py from its true first pose, with the default schedule
    -> (steps, volume).  Shared by the tests: do not write into it"""
    steps, volume = track(cases.frames(name, depth_type)[:n_frames], cases.true_poses(name)[0], depth_type, cases.ORIGIN, cases.DIMS,
                          configs.DENSE_ALIGN["schedule"], None if mutant is None else MUTANTS[mutant])
    volume.setflags(write=False)
    return steps, volume


@functools.lru_cache(maxsize=None)
def mesh_of(name, depth_type):
    """the mesh restatement on the tracked volume, min_weight 1 and strides of MESH_STRIDE"""
    return tsdf_mesh_ref.mesh(tracked(name, depth_type)[1], settings(depth_type)[0], cases.ORIGIN, MESH_STRIDE, MESH_STRIDE)


@functools.lru_cache(maxsize=None)
def view_of(name, depth_type):
    """the raycast restatement of the tracked volume at the TRUE pose of the last frame"""
    pose = cases.true_poses(name)[-1].astype(F).reshape(1, 16)
    return tsdf_raycast_ref.raycast(dict(pose=pose), settings(depth_type)[1], cases.ORIGIN, tracked(name, depth_type)[1], 1,
                                    cases.ROWS, cases.COLS)

"""A float64 restatement of the landmark estimators and of the merger's point initialisation, written from the reference
sources (srrg2_proslam/src/srrg2_proslam/mapping/...) and independent of both the HIP kernels (csrc/mapping.hip) and the C
checker (oracle/proslam_oracle_mapping.c): plain numpy, every quantity in double, matrix inverses and solves by numpy.linalg.

It is a reference for the ARITHMETIC, not a second merger: which correspondence was allowed to update its landmark (appearance
gate, first-come bin blocking) and which measurements were added are read off the result under test (the counters of the map
before and after the frame); for those landmarks the numbers are recomputed here.

    set_transforms            landmarks/landmark_estimator_base.hpp:47-55
    weighted_mean_update      landmarks/landmark_estimator_weighted_mean_impl.cpp:17-40
    ekf_update                landmarks/landmark_estimator_ekf_impl.cpp:26-81, landmarks/filters/point_ekf_base.hpp:63-112,
                              filters/stereo_projective_point_ekf_impl.cpp:23-47, projective_depth_point_ekf_impl.cpp:7-36,
                              projective_point_ekf_impl.cpp:16-43
    smoother_*                landmarks/landmark_estimator_pose_based_smoother_impl.cpp:26-147
    triangulate / unproject   triangulator_rigid_stereo.cpp:60-85, merger_projective_depth_ekf_impl.cpp (the unprojector)
    initialize_landmark       mergers/merger_projective_impl.cpp:283-296, :311-327
"""
import numpy as np

from oracle import binding_mapping as om

GATE_MARGIN = 1e-3  # a float64 gate value within this (relative) of its threshold decides nothing: the landmark is left out


def f64(a):
    return np.asarray(a, dtype=np.float64)


def apply(T, p):
    T = f64(T)
    return T[:3, :3] @ f64(p) + T[:3, 3]


def set_transforms(measurement_in_world, measurement_in_scene):
    """landmark_estimator_base.hpp:49-54"""
    sensor_in_world = f64(measurement_in_world).reshape(4, 4)
    sensor_in_local_map = f64(measurement_in_scene).reshape(4, 4)
    world_in_sensor = np.linalg.inv(sensor_in_world)                # :52
    world_in_local_map = sensor_in_local_map @ world_in_sensor      # :54
    return {"sensor_in_world": sensor_in_world, "world_in_sensor": world_in_sensor, "world_in_local_map": world_in_local_map,
            "sensor_in_local_map": sensor_in_local_map}


def weighted_mean_update(initial_in_world, n_opt, t, landmark_in_sensor):
    """landmark_estimator_weighted_mean_impl.cpp:17-30 -> (coordinates in world, squared distance to the initial ones)"""
    init = f64(initial_in_world)
    update = apply(t["sensor_in_world"], landmark_in_sensor)        # :19-20
    w = float(n_opt) + 1.0                                          # :22
    world = (w * init + update) / (w + 1.0)                         # :24-26
    return world, float(np.sum((world - init) ** 2))                # :29


def ekf_measurement_model(E, dim, s):
    """_computeMeasurementPrediction of the three filters -> (prediction h [dim], jacobian J [dim, 3])"""
    x, y, z = s
    fx, fy, cx, cy = E.fx, E.fy, E.cx, E.cy
    if dim == 4:  # stereo_projective_point_ekf_impl.cpp:23-47
        x_h, y_h = fx * x + cx * z, fy * y + cy * z
        h = np.array([x_h / z, y_h / z, (x_h - E.b_x) / z, (y_h - E.b_y) / z])
        J = np.array([[fx / z, 0.0, -fx * x / z ** 2], [0.0, fy / z, -fy * y / z ** 2],
                      [fx / z, 0.0, -(fx * x - E.b_x) / z ** 2], [0.0, fy / z, -(fy * y - E.b_y) / z ** 2]])
        return h, J
    h = [fx / z * x + cx, fy / z * y + cy]
    J = [[fx / z, 0.0, -fx * x / z ** 2], [0.0, fy / z, -fy * y / z ** 2]]
    if dim == 3:  # projective_depth_point_ekf_impl.cpp:7-36: the third row measures the depth itself
        h.append(z)
        J.append([0.0, 0.0, 1.0])
    return np.array(h), np.array(J)


def ekf_update(E, initial_in_world, covariance, t, measurement):
    """landmark_estimator_ekf_impl.cpp:26-72 -> dict(world, covariance, z_sensor, covariance_norm2, distance2)"""
    dim = int(E.measurement_dim)
    R = np.eye(dim) * E.minimum_state_element_covariance            # :26-27
    state = f64(initial_in_world)
    P = f64(covariance).reshape(3, 3).copy()
    for i in range(3):                                              # :46-48
        P[i, i] = max(P[i, i], E.minimum_state_element_covariance)
    F = t["world_in_sensor"][:3, :3]                                # point_ekf_base.hpp:69-75
    P = F @ P @ F.T
    state = apply(t["world_in_sensor"], state)
    h, J = ekf_measurement_model(E, dim, state)                     # :89
    K = P @ J.T @ np.linalg.inv(R + J @ P @ J.T)                    # :98-102
    state = state + K @ (f64(measurement)[:dim] - h)                # :106
    P = (np.eye(3) - K @ J) @ P                                     # :110-111
    world = apply(t["sensor_in_world"], state)                      # landmark_estimator_ekf_impl.cpp:66-67
    return {"world": world, "covariance": P, "z_sensor": float(state[2]), "covariance_norm2": float(np.sum(P * P)),
            "distance2": float(np.sum((world - f64(initial_in_world)) ** 2))}


def smoother_history(m, idx, poses):
    """the measurement history of landmark idx as float64 arrays + the world_in_sensor / sensor_in_world rows of its frames"""
    n = int(m.n_meas[idx])
    h = m.meas[idx, :n]
    fr = h["frame"].astype(np.int64)
    return {"uv": f64(h["point_in_image"][:, :2]), "depth": f64(h["point_in_camera"][:, 2]), "point_in_camera": f64(h["point_in_camera"]),
            "world_in_sensor": f64(poses["world_in_sensor"][fr]).reshape(n, 3, 4), "sensor_in_world": f64(poses["sensor_in_world"][fr]).reshape(n, 3, 4)}


def smoother_mean_in_world(hist):
    """_setMeanCoordinatesInWorld, landmark_estimator_pose_based_smoother_impl.cpp:139-147"""
    S = hist["sensor_in_world"]
    return (np.einsum("nij,nj->ni", S[:, :, :3], hist["point_in_camera"]) + S[:, :, 3]).mean(axis=0)


def smoother_normal_equations(E, hist, world):
    """one pass over the measurements, :49-103 -> (H, b, chi2, number of outliers)"""
    Km = f64(list(E.camera_matrix)).reshape(3, 3)
    kernel = float(E.maximum_reprojection_error_pixels_squared)
    H, b, chi2, outliers = np.zeros((3, 3)), np.zeros(3), 0.0, 0
    for k in range(len(hist["uv"])):
        omega = np.diag([1.0, 1.0, 10.0])                           # :56-57
        W = hist["world_in_sensor"][k]
        pc = W[:, :3] @ world + W[:, 3]                             # :60
        if pc[2] <= 0:                                              # :61-64
            outliers += 1
            continue
        ph = Km @ pc                                                # :65
        c = ph[2]
        e = np.array([ph[0] / c - hist["uv"][k, 0], ph[1] / c - hist["uv"][k, 1], c - hist["depth"][k]])  # :72-74
        e2 = float(e @ omega @ e)                                   # :77
        chi2 += e2
        if e2 > kernel:                                             # :81-84
            omega = omega * (kernel / e2)
            outliers += 1
        Jh = np.array([[1.0 / c, 0.0, -ph[0] / c ** 2], [0.0, 1.0 / c, -ph[1] / c ** 2], [0.0, 0.0, 1.0]])  # :91-95
        J = Jh @ (Km @ W[:, :3])                                    # :87, :97
        H += J.T @ omega @ J                                        # :101-102
        b += J.T @ omega @ e
    return H, b, chi2, outliers


def smoother_step(E, hist, world):
    """the Gauss-Newton step at `world` (:106)"""
    H, b, _, _ = smoother_normal_equations(E, hist, f64(world))
    return np.linalg.solve(H, -b)


def smoother_run(E, hist, initial_in_world):
    """the loop :45-117 -> (world, number of inliers, True when it ended by the chi2 criterion)"""
    world, previous, inliers = f64(initial_in_world).copy(), 0.0, 0
    for _ in range(int(E.maximum_number_of_iterations)):
        H, b, chi2, outliers = smoother_normal_equations(E, hist, world)
        world = world + np.linalg.solve(H, -b)
        inliers = len(hist["uv"]) - outliers
        if abs(chi2 - previous) < E.convergence_criterion_minimum_chi2_delta:
            return world, inliers, True
        previous = chi2
    return world, inliers, False


def triangulate(tp, z):
    """triangulateRectifiedMidpoint (triangulator_rigid_stereo.cpp:60-85) -> point in the camera or None"""
    x_l, y_l, x_r, y_r = [float(v) for v in z[:4]]
    if x_l - x_r < tp.minimum_disparity_pixels:
        return None
    depth = float(tp.infinity_depth_meters)
    if x_l > x_r:
        depth = float(tp.b_x) / (x_l - x_r)
    return np.array([(x_l - tp.cx) / tp.fx * depth, ((y_l + y_r) / 2.0 - tp.cy) / tp.fy * depth, depth])


def unproject(P, z):
    """the depth merger's unprojection of (u, v, d) -> point in the camera or None"""
    u, v, d = [float(x) for x in z[:3]]
    if not d > 0.0:
        return None
    return np.array([(u - P.cx) / P.fx * d, (v - P.cy) / P.fy * d, d])


def point_in_camera(P, z):
    return unproject(P, z) if P.variant == om.MERGER_DEPTH_EKF else triangulate(P.triangulator, z)


def initialize_landmark(t, p_cam):
    """_initializeLandmark (merger_projective_impl.cpp:318-320) and the move into the scene frame (:293-294)
    -> (state in world, covariance, coordinates in the scene)"""
    return apply(t["sensor_in_world"], p_cam), np.eye(3), apply(t["sensor_in_local_map"], p_cam)


class Deviations:
    """largest absolute deviation of a result from the float64 values, per quantity, over everything check_frame has seen"""

    def __init__(self):
        self.state = self.covariance = self.coords = self.step = 0.0
        self.checked = self.left_out = self.added = 0
        self.reasons = {}

    def leave_out(self, reason):
        self.left_out += 1
        self.reasons[reason] = self.reasons.get(reason, 0) + 1

    def share_left_out(self):
        return self.left_out / max(self.checked + self.left_out, 1)

    def merge(self, o):
        for q in ("state", "covariance", "coords", "step"):
            setattr(self, q, max(getattr(self, q), getattr(o, q)))
        self.checked, self.left_out, self.added = self.checked + o.checked, self.left_out + o.left_out, self.added + o.added
        for k, v in o.reasons.items():
            self.reasons[k] = self.reasons.get(k, 0) + v

    def __repr__(self):
        return "state %.3g covariance %.3g coords %.3g step %.3g | %d checked, %d added, %d left out %s" % (
            self.state, self.covariance, self.coords, self.step, self.checked, self.added, self.left_out, self.reasons)


def _near(value, threshold):
    return abs(value - threshold) <= GATE_MARGIN * abs(threshold)


def check_frame(P, before, after, poses, frame, measurement_in_world, measurement_in_scene, measurement, measurement_desc, corr,
                scene_index_map=None, dev=None):
    """One merged frame: `before` / `after` are the map (om.Map layout) before and after it, `poses` the pose table after it.
    Structural facts (counters, flags, descriptors, history rows) are asserted here; numeric deviations from the float64 values
    are accumulated in `dev` (the caller compares them with its tolerances)."""
    dev = dev if dev is not None else Deviations()
    E = P.estimator
    t = set_transforms(measurement_in_world, measurement_in_scene)
    z_all = np.asarray(measurement, np.float32).reshape(-1, int(E.measurement_dim))
    max_d2 = float(E.maximum_distance_geometry_meters_squared)

    def coords_dev(idx):
        return float(np.abs(f64(after.coords[idx, :3]) - apply(t["world_in_local_map"], after.state[idx, :3])).max())

    for c in corr:
        s, m = int(c["fixed_idx"]), int(c["moving_idx"])
        if scene_index_map is not None:
            s = int(scene_index_map[s])
        z = z_all[m]
        if E.type == om.EST_SMOOTHER:
            if int(after.n_meas[s]) != int(before.n_meas[s]) + 1:
                continue  # the estimator was not run on this landmark
            n = int(after.n_meas[s])
            row = after.meas[s, n - 1]
            assert np.array_equal(row["point_in_image"], z[:3]) and int(row["frame"]) == frame, ("history row", s)
            lis = triangulate(P.triangulator, z)
            assert lis is not None and np.abs(f64(row["point_in_camera"]) - lis).max() <= 1e-4 * max(1.0, abs(lis[2])), ("point_in_camera", s)
            hist = smoother_history(after, s, poses)
            if n < E.minimum_number_of_measurements_for_optimization:  # :29-42
                mean = smoother_mean_in_world(hist)
                d2 = float(np.sum((mean - f64(before.state[s, :3])) ** 2))
                if _near(d2, max_d2):
                    dev.leave_out("geometry gate")
                    continue
                assert bool(after.inlier[s]) == (d2 < max_d2), ("averaging gate", s, d2)
                if after.inlier[s]:
                    dev.checked += 1
                    assert int(after.n_opt[s]) == n
                    dev.state = max(dev.state, float(np.abs(f64(after.state[s, :3]) - mean).max()))
                    dev.coords = max(dev.coords, coords_dev(s))
                    assert np.array_equal(after.desc[s], measurement_desc[m]), ("descriptor", s)
                continue
            _, _, ended = smoother_run(E, hist, before.state[s, :3])
            if not ended:
                dev.leave_out("float64 smoother out of iterations")
                continue
            dev.checked += 1
            if after.inlier[s]:  # :120-124 the optimised position was taken
                assert int(after.n_opt[s]) == int(before.n_opt[s]) + 1
                dev.step = max(dev.step, float(np.abs(smoother_step(E, hist, after.state[s, :3])).max()))
                assert np.array_equal(after.desc[s], measurement_desc[m]), ("descriptor", s)
            else:  # :128-132 reset to the mean
                assert int(after.n_opt[s]) == int(before.n_opt[s])
                dev.state = max(dev.state, float(np.abs(f64(after.state[s, :3]) - smoother_mean_in_world(hist)).max()))
            dev.coords = max(dev.coords, coords_dev(s))
            continue
        if int(after.n_opt[s]) != int(before.n_opt[s]) + 1:
            continue  # gated, blocked by its bin, or refused by the estimator
        assert after.inlier[s] == 1 and np.array_equal(after.desc[s], measurement_desc[m]), ("merged landmark", s)
        if E.type == om.EST_WEIGHTED_MEAN:
            lis = triangulate(P.triangulator, z)
            assert lis is not None
            world, d2 = weighted_mean_update(before.state[s, :3], before.n_opt[s], t, lis)
            if _near(d2, max_d2):
                dev.leave_out("geometry gate")
                continue
            assert d2 <= max_d2, ("updated against the float64 geometry gate", s, d2)
            assert np.array_equal(after.covariance[s], before.covariance[s])
        else:
            r = ekf_update(E, before.state[s, :3], before.covariance[s], t, z)
            if _near(r["distance2"], max_d2) or _near(r["covariance_norm2"], E.maximum_covariance_norm_squared):
                dev.leave_out("geometry / covariance gate")
                continue
            assert r["z_sensor"] > 0 and r["covariance_norm2"] <= E.maximum_covariance_norm_squared and r["distance2"] <= max_d2, ("updated against a float64 gate", s, r)
            world = r["world"]
            dev.covariance = max(dev.covariance, float(np.abs(f64(after.covariance[s]).reshape(3, 3) - r["covariance"]).max()))
        dev.checked += 1
        dev.state = max(dev.state, float(np.abs(f64(after.state[s, :3]) - world).max()))
        dev.coords = max(dev.coords, coords_dev(s))

    # ---- added points: rows before.n_points .. after.n_points, each created from the measurement with its descriptor ----
    if after.n_points > before.n_points:
        lut = {bytes(d): i for i, d in enumerate(np.asarray(measurement_desc))}
        for idx in range(before.n_points, after.n_points):
            i = lut[bytes(after.desc[idx])]
            p = point_in_camera(P, z_all[i])
            assert p is not None, ("added from an invalid measurement", idx)
            state, cov, coords = initialize_landmark(t, p)
            assert after.inlier[idx] == 1 and after.n_opt[idx] == 0
            assert np.array_equal(f64(after.covariance[idx]).reshape(3, 3), cov)
            if after.max_measurements > 0:
                row = after.meas[idx, 0]
                assert int(after.n_meas[idx]) == 1 and int(row["frame"]) == frame and np.array_equal(row["point_in_image"], z_all[i, :3])
            dev.added += 1
            dev.state = max(dev.state, float(np.abs(f64(after.state[idx, :3]) - state).max()))
            dev.coords = max(dev.coords, float(np.abs(f64(after.coords[idx, :3]) - coords).max()), coords_dev(idx))
    return dev

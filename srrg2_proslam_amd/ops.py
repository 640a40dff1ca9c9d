"""Python host layer over the C-ABI (include/proslam_hip.h).

torch is used for device memory and streams only (plumbing); every operator below is a thin
call into libproslam_hip.so.  Host-array entry points mirror what a srrg2 plugin adapter calls
once per compute(); `*_batch` entry points keep B independent frames resident in HBM.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib, _lib_dense_align, _lib_normals, _lib_tsdf, _lib_tsdf_mesh, _lib_tsdf_raycast, configs
from ._lib import ProslamHipError, StereoBatch, StereoParams, TriangulatorParams

CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])


def _check(ctx, rc, what):
    if rc < 0:
        lib = _lib.load()
        msg = lib.prs_last_error(ctx._h) if ctx is not None and ctx._h else b""
        raise ProslamHipError(rc, "%s: %s (%s)" % (what, lib.prs_status_string(rc).decode(), (msg or b"").decode()))
    return rc


def _run(ctx, entry, *args):
    """call the entry point `entry` of the library on the context: its status, ProslamHipError on a failure"""
    return _check(ctx, getattr(_lib.load(), entry)(ctx._h, *args), entry)


def _run_normals(ctx, entry, *args):
    """_run for an entry point of the second header (include/proslam_hip_normals.h, bound by _lib_normals)"""
    return _check(ctx, getattr(_lib_normals.load(), entry)(ctx._h, *args), entry)


def _run_tsdf(ctx, entry, *args):
    """_run for an entry point of the third header (include/proslam_hip_tsdf.h, bound by _lib_tsdf)"""
    return _check(ctx, getattr(_lib_tsdf.load(), entry)(ctx._h, *args), entry)


def _run_tsdf_raycast(ctx, entry, *args):
    """_run for an entry point of the fourth header (include/proslam_hip_tsdf_raycast.h, bound by _lib_tsdf_raycast)"""
    return _check(ctx, getattr(_lib_tsdf_raycast.load(), entry)(ctx._h, *args), entry)


def _run_dense_align(ctx, entry, *args):
    """_run for an entry point of the fifth header (include/proslam_hip_dense_align.h, bound by _lib_dense_align)"""
    return _check(ctx, getattr(_lib_dense_align.load(), entry)(ctx._h, *args), entry)


def _run_tsdf_mesh(ctx, entry, *args):
    """_run for an entry point of the sixth header (include/proslam_hip_tsdf_mesh.h, bound by _lib_tsdf_mesh)"""
    return _check(ctx, getattr(_lib_tsdf_mesh.load(), entry)(ctx._h, *args), entry)


class Context:
    """prs_context: one device, one stream, scratch. Not re-entrant (like the reference's finders).

    Stream policy: the `*_batch` operators read and write torch tensors, whose fills and copies run on torch's current
    stream; a context that launched on its own (non-blocking) stream would not be ordered against them.  By default the
    context therefore enqueues on torch's current stream of `device` (stream="torch").  stream="own" keeps the
    context's private stream: the caller then orders the two streams itself (events) or only uses host-array entry
    points, which synchronise internally."""

    def __init__(self, device=0, stream="torch"):
        lib = _lib.load()
        h = C.c_void_p()
        rc = lib.prs_context_create(int(device), C.byref(h))
        if rc < 0:
            raise ProslamHipError(rc, "prs_context_create(device=%d): %s" % (device, lib.prs_status_string(rc).decode()))
        self._h = h
        self.device = int(device)
        self._children = weakref.WeakSet()  # handles that hold a pointer to this context
        if stream == "torch":
            self.use_torch_stream()
        elif stream != "own":
            raise ValueError("stream must be 'torch' or 'own'")

    def close(self):
        if getattr(self, "_h", None):
            for child in list(self._children):  # a finder handle must never outlive its context
                child.close()
            # (guard mode: the damaged bands latched when the context went, which it has printed; else 0)
            self.close_status = _lib.load().prs_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self):
        """enqueue on torch's current stream so torch ops and these kernels are ordered"""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        _check(self, _lib.load().prs_context_set_stream(self._h, C.c_void_p(s)), "prs_context_set_stream")

    def synchronize(self):
        _check(self, _lib.load().prs_context_synchronize(self._h), "prs_context_synchronize")

    def set_bruteforce_dense_phase(self, mode):
        """BF_DENSE_POPCOUNT / BF_DENSE_MATRIX_WHEN_FULL (default) / BF_DENSE_MATRIX: which kernels score the brute-force matcher's
        N_f x N_m pairs (prs_context_set_bruteforce_dense_phase; same results, the matrix cores pay only when candidates are rare)"""
        _check(self, _lib.load().prs_context_set_bruteforce_dense_phase(self._h, int(mode)), "prs_context_set_bruteforce_dense_phase")

    def enable_timing(self, on=True):
        """HIP-event timing of the aligner's two kernels inside align_batch (measurement only)"""
        _check(self, _lib.load().prs_context_enable_timing(self._h, 1 if on else 0), "prs_context_enable_timing")

    def align_timing(self):
        """-> dict(search_ms, gn_ms, search_launches, gn_launches) accumulated since enable_timing()"""
        a, b, c, d = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int64(0)
        _check(self, _lib.load().prs_context_get_align_timing(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "prs_context_get_align_timing")
        return {"search_ms": a.value, "gn_ms": b.value, "search_launches": c.value, "gn_launches": d.value}

    def search_reuse(self):
        """-> (hits, misses): queries the later searches of the last finished batch settled from the query cache / scanned again"""
        h, m = C.c_int64(0), C.c_int64(0)
        _check(self, _lib.load().prs_context_get_search_reuse(self._h, C.byref(h), C.byref(m)), "prs_context_get_search_reuse")
        return h.value, m.value

    def guard_regions(self):
        """guard mode (PRS_GUARD_FILL=00 / ff when the context was created): the library's live blocks on this context in allocation
        order -> [dict(name, user, bytes, tail_bytes, pinned)]; ProslamHipError on a context that is not in guard mode"""
        lib = _lib.load()
        n = _check(self, lib.prs_context_guard_regions(self._h, None, 0), "prs_context_guard_regions")
        out = (_lib.GuardRegion * max(n, 1))()
        n = min(n, _check(self, lib.prs_context_guard_regions(self._h, out, n), "prs_context_guard_regions"))
        return [dict(name=r.name.decode(), user=r.user or 0, bytes=r.bytes, tail_bytes=r.tail_bytes, pinned=bool(r.pinned)) for r in out[:n]]

    def guard_check(self, report=False):
        """guard mode: synchronises, looks at the bands of every live block and -> the number of damaged (block, side) pairs, those
        latched from freed blocks included; report=True -> (count, ["name front|tail offset", ...])"""
        text = C.create_string_buffer(1 << 16)
        n = _check(self, _lib.load().prs_context_guard_check(self._h, text, len(text)), "prs_context_guard_check")
        return (n, text.value.decode().splitlines()) if report else n

    def align_round_timing(self):
        """-> (search_ms[16], gn_ms[16], batches): the timed launches by round of the batch (mean per batch = value / batches)"""
        a, b, n = (C.c_double * 16)(), (C.c_double * 16)(), C.c_int64(0)
        _check(self, _lib.load().prs_context_get_align_round_timing(self._h, a, b, C.byref(n)), "prs_context_get_align_round_timing")
        return list(a), list(b), n.value


# =================================================================================================
# dispatch plans (tests and tools): which kernels a launch would run, without a device
# =================================================================================================
def dispatch_env(ctx=None, **fields):
    """prs_dispatch_env: a live context's (its real CU count and knobs, the brute-force switches from the environment as it is now),
    or 256 CUs with every knob at its default; fields override either"""
    env = _lib.DispatchEnv(cus=256, bf_mfma=1, bf_two_workgroups=-1)  # (PRS_BF_DENSE_MATRIX_WHEN_FULL)
    if ctx is not None:
        _check(ctx, _lib.load().prs_context_get_dispatch_env(ctx._h, C.byref(env)), "prs_context_get_dispatch_env")
    for k, v in fields.items():
        setattr(env, k, int(v))
    return env


def dispatch_kernel_names(family):
    """every kernel a plan of the family (_lib.DISPATCH_*) can name, as a kernel trace prints them"""
    lib, names = _lib.load(), []
    while lib.prs_dispatch_kernel_name(family, len(names)) is not None:
        names.append(lib.prs_dispatch_kernel_name(family, len(names)).decode())
    return names


def _plan(family, entry, *args):
    """-> dict(status, message, kernels, launches=[dict(kernel, grid_x, grid_y, block, lds)], + the family's facts by name)"""
    plan = _lib.DispatchPlan()
    rc = getattr(_lib.load(), entry)(*[a if isinstance(a, int) else C.byref(a) for a in args], C.byref(plan))
    if rc != 0:
        raise ProslamHipError(rc, entry)
    launches = [dict(kernel=l.kernel.decode(), grid_x=l.grid_x, grid_y=l.grid_y, block=l.block, lds=l.lds_bytes) for l in plan.launch[:plan.n_launches]]
    out = dict(status=plan.status, message=plan.message.decode() if plan.message else None, launches=launches,
               kernels=[l["kernel"] for l in launches])
    out.update(zip(_lib.PLAN_FACTS[family], plan.fact))
    return out


def stereo_plan(params, batch, env):
    """prs_stereo_plan(prs_stereo_params, prs_stereo_batch descriptor, prs_dispatch_env)"""
    return _plan(_lib.DISPATCH_STEREO, "prs_stereo_plan", params, batch, env)


def align_plan(finder_params, aligner_params_, batch, env, mode=_lib.MODE_ALIGN):
    return _plan(_lib.DISPATCH_ALIGN, "prs_align_plan", finder_params, aligner_params_, batch, int(mode), env)


def bruteforce_plan(params, batch, env):
    return _plan(_lib.DISPATCH_BRUTEFORCE, "prs_bruteforce_plan", params, batch, env)


def merge_plan(params, batch, env):
    return _plan(_lib.DISPATCH_MERGE, "prs_merge_plan", params, batch, env)


def stereo_params(cfg_matcher, image_rows, image_cols=0):
    """image_cols is reserved (ignored)"""
    return StereoParams(
        float(cfg_matcher["maximum_descriptor_distance"]),
        float(cfg_matcher["maximum_distance_ratio_to_second_best"]),
        float(cfg_matcher["minimum_matching_ratio"]),
        int(cfg_matcher["maximum_disparity_pixels"]),
        int(cfg_matcher["epipolar_line_thickness_pixels"]),
        int(image_rows),
        int(image_cols),
    )


def triangulator_params(cfg):
    cam, tri = cfg["camera"], cfg["triangulator"]
    return TriangulatorParams(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fx"] * cam["baseline_m"],
                              tri["minimum_disparity_pixels"], tri["infinity_depth_meters"])


def _np(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.reshape(shape)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def stereo_match(ctx, params, uv_left, desc_left, uv_right, desc_right):
    """host arrays, one frame -> (correspondences [CORR_DTYPE], warning bits)
    fixed = left keypoints, moving = right keypoints (raw_data_preprocessor_stereo_projective.cpp:99-102)"""
    uvl, uvr = _np(uv_left, np.float32, (-1, 2)), _np(uv_right, np.float32, (-1, 2))
    dl, dr = _np(desc_left, np.uint8, (-1, 32)), _np(desc_right, np.uint8, (-1, 32))
    nl, nr = uvl.shape[0], uvr.shape[0]
    out = np.zeros(max(nl, 1), dtype=CORR_DTYPE)
    n = C.c_int32(0)
    rc = _lib.load().prs_stereo_match(ctx._h, C.byref(params), _p(uvl), _p(dl), nl, _p(uvr), _p(dr), nr, _p(out), out.shape[0], C.byref(n))
    _check(ctx, rc, "prs_stereo_match")
    return out[: n.value].copy(), rc


def triangulate(ctx, params, uvuv):
    """host arrays -> (xyz [n,3], valid [n])"""
    uvuv = _np(uvuv, np.float32, (-1, 4))
    n = uvuv.shape[0]
    xyz = np.zeros((max(n, 1), 3), dtype=np.float32)
    valid = np.zeros(max(n, 1), dtype=np.uint8)
    rc = _lib.load().prs_triangulate(ctx._h, C.byref(params), _p(uvuv), n, _p(xyz), _p(valid))
    _check(ctx, rc, "prs_triangulate")
    return xyz[:n].copy(), valid[:n].copy()


class StereoFrames:
    """B stereo pairs resident in HBM (torch tensors own the memory) + the outputs of the
    batched matcher with its fused adaptor/triangulator epilogue."""

    def __init__(self, device, batch, stride, epilogue=True):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.stride = int(batch), int(stride)
        self.left_kp = torch.zeros((batch, stride, 2), dtype=torch.float32, device=dev)
        self.right_kp = torch.zeros((batch, stride, 2), dtype=torch.float32, device=dev)
        self.left_desc = torch.zeros((batch, stride, 32), dtype=torch.uint8, device=dev)
        self.right_desc = torch.zeros((batch, stride, 32), dtype=torch.uint8, device=dev)
        self.n_left = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.n_right = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.matches = torch.zeros((batch, stride, 3), dtype=torch.int32, device=dev)  # prs_corr as 3 x 32 bit
        self.n_matches = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.epilogue = epilogue
        if epilogue:
            self.fixed_uvuv = torch.zeros((batch, stride, 4), dtype=torch.float32, device=dev)
            self.fixed_desc = torch.zeros((batch, stride, 32), dtype=torch.uint8, device=dev)
            self.n_fixed = torch.zeros((batch,), dtype=torch.int32, device=dev)
            self.fixed_xyz = torch.zeros((batch, stride, 4), dtype=torch.float32, device=dev)

    def upload(self, b, uv_left, desc_left, uv_right, desc_right):
        import torch
        nl, nr = len(uv_left), len(uv_right)
        if nl:
            self.left_kp[b, :nl] = torch.from_numpy(np.ascontiguousarray(uv_left, dtype=np.float32))
            self.left_desc[b, :nl] = torch.from_numpy(np.ascontiguousarray(desc_left, dtype=np.uint8))
        if nr:
            self.right_kp[b, :nr] = torch.from_numpy(np.ascontiguousarray(uv_right, dtype=np.float32))
            self.right_desc[b, :nr] = torch.from_numpy(np.ascontiguousarray(desc_right, dtype=np.uint8))
        self.n_left[b] = nl
        self.n_right[b] = nr

    def descriptor(self, tri_params=None):
        d = StereoBatch()
        d.batch, d.stride = self.batch, self.stride
        d.left_kp, d.left_desc, d.n_left = self.left_kp.data_ptr(), self.left_desc.data_ptr(), self.n_left.data_ptr()
        d.right_kp, d.right_desc, d.n_right = self.right_kp.data_ptr(), self.right_desc.data_ptr(), self.n_right.data_ptr()
        d.matches, d.n_matches, d.status = self.matches.data_ptr(), self.n_matches.data_ptr(), self.status.data_ptr()
        if self.epilogue and tri_params is not None:
            d.fixed_uvuv, d.fixed_desc = self.fixed_uvuv.data_ptr(), self.fixed_desc.data_ptr()
            d.n_fixed, d.fixed_xyz = self.n_fixed.data_ptr(), self.fixed_xyz.data_ptr()
            d.triangulator = C.pointer(tri_params)
        return d

    def matches_of(self, b):
        """download frame b's correspondences as a CORR_DTYPE array"""
        n = int(self.n_matches[b].item())
        raw = self.matches[b, :n].cpu().numpy()
        out = np.zeros(n, dtype=CORR_DTYPE)
        out["fixed_idx"] = raw[:, 0]
        out["moving_idx"] = raw[:, 1]
        out["response"] = raw[:, 2].view(np.float32)
        return out


def stereo_match_batch(ctx, params, frames, tri_params=None):
    """enqueue the batched matcher on the context stream (asynchronous)"""
    d = frames.descriptor(tri_params)
    return _run(ctx, "prs_stereo_match_batch", C.byref(params), C.byref(d))


# =================================================================================================
# projective correspondence finder + Gauss-Newton aligner
# =================================================================================================
from ._lib import AlignBatch, AlignerParams, AlignResult, PcfParams, PcfState, Projector  # noqa: E402


def pcf_params(cfg, **overrides):
    """prs_pcf_params from a configs.* dictionary (projective_finder + projector + camera)"""
    cam, pr = cfg["camera"], cfg["projector"]
    f = dict(cfg["projective_finder"])
    f.update(overrides)
    proj = Projector(cam["fx"], cam["fy"], cam["cx"], cam["cy"], int(cam["cols"]), int(cam["rows"]),
                     pr["range_min"], pr["range_max"])
    return PcfParams(f["maximum_descriptor_distance"], f["maximum_distance_ratio_to_second_best"],
                     f["minimum_matching_ratio"], f["minimum_descriptor_distance"],
                     f["descriptor_distance_step_size_pixels"], int(f["maximum_search_radius_pixels"]),
                     int(f["minimum_search_radius_pixels"]), int(f["search_radius_step_size_pixels"]),
                     int(f["minimum_number_of_iterations"]), f["maximum_estimate_change_norm_for_convergence"],
                     int(f["number_of_solver_iterations_per_projection"]), int(f["search_type"]), proj)


def aligner_params(cfg, mean_disparity=-1.0, stop_at_fixed_point=1, **overrides):
    """prs_aligner_params from a configs.* dictionary; mean_disparity < 0 = computed on the device"""
    cam, al = cfg["camera"], dict(cfg["aligner"])
    al.update(overrides)
    p = AlignerParams()
    p.factor_type = int(al["factor_type"])
    p.fx, p.fy, p.cx, p.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    p.image_cols, p.image_rows = cam["cols"], cam["rows"]
    p.baseline_left_in_right_px[0] = -cam["fx"] * cam.get("baseline_m", 0.0)  # K * t_left_in_right
    for i in range(3):
        p.diagonal_info[i] = al["diagonal_info"][i]
    p.chi_threshold = al["chi_threshold"]
    p.enable_inverse_depth_weighting = int(al["enable_inverse_depth_weighting"])
    p.mean_disparity = mean_disparity
    p.damping = al["damping"]
    p.max_iterations = int(al["max_iterations"])
    p.min_num_inliers = int(al["min_num_inliers"])
    p.min_num_correspondences = int(al["min_num_correspondences"])
    p.stop_at_fixed_point = int(stop_at_fixed_point)
    # MultiAligner3DQR flags of the RGB-D configurations (icl.conf:50-64, tum.conf:90-104)
    p.enable_inlier_only_runs = int(al.get("enable_inlier_only_runs", 0))
    p.keep_only_inlier_correspondences = int(al.get("keep_only_inlier_correspondences", 0))
    p.inlier_only_iterations = int(al.get("inlier_only_iterations", 0))
    # readings of the external srrg2_solver arithmetic (0 = shipped; include/proslam_hip.h)
    p.kernel_weight_form = int(al.get("kernel_weight_form", 0))
    p.damping_form = int(al.get("damping_form", 0))
    p.translation_weight_form = int(al.get("translation_weight_form", 0))
    p.step_norm_exit = float(al.get("step_norm_exit", 0.0))  # opt-in: does less work than the reference
    if al.get("sensor_in_robot") is not None:
        set_sensor_in_robot(p, al["sensor_in_robot"])
    if al.get("motion_prior_info") is not None:
        set_motion_prior(p, al["motion_prior_info"])
    return p


def set_sensor_in_robot(p, S):
    """...WithSensor factor variants (aligner_slice_processor_projective.h:80-83): X is the robot's movingInFixed"""
    p.with_sensor = 1
    for i, v in enumerate(np.asarray(S, np.float32).reshape(16)):
        p.sensor_in_robot[i] = float(v)
    return p


def set_motion_prior(p, info=(1.0,) * 6):
    """AlignerSliceMotionModel3D stand-in (kitti.conf:747-772): prior on movingInFixed with diagonal information"""
    p.enable_motion_prior = 1
    for i in range(6):
        p.motion_prior_info[i] = float(info[i])
    return p


def info_scale_from_nopt(n_opt):
    n_opt = np.ascontiguousarray(n_opt, dtype=np.uint32)
    out = np.zeros(max(len(n_opt), 1), dtype=np.float32)
    _lib.load().prs_info_scale_from_nopt(_p(n_opt), len(n_opt), _p(out))
    return out[: len(n_opt)].copy()


def gn_step(ctx, H, b, damping, X, damping_form=0):
    H, b = _np(H, np.float32, (36,)), _np(b, np.float32, (6,))
    X = _np(X, np.float32, (16,)).copy()
    rc = _lib.load().prs_gn_step_ex(ctx._h, _p(H), _p(b), float(damping), int(damping_form), _p(X))
    _check(ctx, rc, "prs_gn_step")
    return X.reshape(4, 4), rc


class ProjectiveFinder:
    """host-array handle mirroring CorrespondenceFinderProjective{KDTree,Square,Circle,Rhombus}:
    set_fixed / set_moving / set_local_map_in_sensor / compute, state carried across calls"""

    def __init__(self, ctx, params):
        self.ctx = ctx
        h = C.c_void_p()
        _check(ctx, _lib.load().prs_pcf_create(ctx._h, C.byref(params), C.byref(h)), "prs_pcf_create")
        self._h = h
        self._n_fixed = 0
        ctx._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                _lib.load().prs_pcf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        _check(self.ctx, _lib.load().prs_pcf_set_params(self._h, C.byref(params)), "prs_pcf_set_params")

    def set_fixed(self, coords, desc):
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        if coords.ndim != 2:
            coords = coords.reshape(-1, 2)
        d = _np(desc, np.uint8, (-1, 32))
        self._n_fixed = coords.shape[0]
        _check(self.ctx, _lib.load().prs_pcf_set_fixed(self._h, _p(coords), coords.shape[1], _p(d), coords.shape[0]), "prs_pcf_set_fixed")

    def set_moving(self, xyz, desc, info_scale=None):
        xyz = _np(xyz, np.float32, (-1, 3))
        d = _np(desc, np.uint8, (-1, 32))
        sc = None if info_scale is None else _np(info_scale, np.float32, (-1,))
        _check(self.ctx, _lib.load().prs_pcf_set_moving(self._h, _p(xyz), None if sc is None else _p(sc), _p(d), xyz.shape[0]), "prs_pcf_set_moving")

    def set_local_map_in_sensor(self, T):
        T = _np(T, np.float32, (16,))
        _check(self.ctx, _lib.load().prs_pcf_set_local_map_in_sensor(self._h, _p(T)), "prs_pcf_set_local_map_in_sensor")

    def set_search_radius(self, r):
        _check(self.ctx, _lib.load().prs_pcf_set_search_radius(self._h, int(r)), "prs_pcf_set_search_radius")

    def set_descriptor_distance(self, d):
        _check(self.ctx, _lib.load().prs_pcf_set_descriptor_distance(self._h, float(d)), "prs_pcf_set_descriptor_distance")

    def state(self):
        st = PcfState()
        _check(self.ctx, _lib.load().prs_pcf_get_state(self._h, C.byref(st)), "prs_pcf_get_state")
        return st

    @property
    def search_radius(self):
        return int(self.state().search_radius_pixels)

    @property
    def descriptor_distance(self):
        return float(self.state().descriptor_distance)

    @property
    def iteration(self):
        return int(self.state().current_iteration)

    @property
    def has_converged(self):
        return bool(self.state().has_converged)

    @property
    def num_recomputes(self):
        return int(self.state().num_recomputes)

    def local_map_in_sensor(self):
        return np.array(self.state().local_map_in_sensor, dtype=np.float32).reshape(4, 4)

    def compute(self):
        out = np.zeros(max(self._n_fixed, 1), dtype=CORR_DTYPE)
        n = C.c_int32(0)
        rc = _lib.load().prs_pcf_compute(self._h, _p(out), out.shape[0], C.byref(n))
        _check(self.ctx, rc, "prs_pcf_compute")
        return out[: n.value].copy(), rc

    def set_motion_prior_mean(self, Z):
        """mean of the motion prior (None = identity)"""
        z = None if Z is None else _np(Z, np.float32, (16,))
        _check(self.ctx, _lib.load().prs_pcf_set_motion_prior_mean(self._h, None if z is None else _p(z)), "prs_pcf_set_motion_prior_mean")

    def align(self, params, X_init, prior=None):
        """the whole per-frame loop; returns (X [4,4], correspondences, prs_align_result, warnings)"""
        X0 = _np(X_init, np.float32, (16,))
        X = np.zeros(16, dtype=np.float32)
        out = np.zeros(max(self._n_fixed, 1), dtype=CORR_DTYPE)
        n = C.c_int32(0)
        res = AlignResult()
        pr = None if prior is None else _np(np.concatenate([np.ravel(prior[0]), np.ravel(prior[1])]), np.float32, (42,))
        rc = _lib.load().prs_pcf_align(self._h, C.byref(params), _p(X0), None if pr is None else _p(pr), _p(X), _p(out), out.shape[0], C.byref(n), C.byref(res))
        _check(self.ctx, rc, "prs_pcf_align")
        return X.reshape(4, 4), out[: n.value].copy(), res, rc

    def linearize(self, params, X, corr):
        X = _np(X, np.float32, (16,))
        corr = np.ascontiguousarray(corr, dtype=CORR_DTYPE)
        res = AlignResult()
        rc = _lib.load().prs_pcf_linearize(self._h, C.byref(params), _p(X), _p(corr), len(corr), C.byref(res))
        _check(self.ctx, rc, "prs_pcf_linearize")
        return res


class AlignFrames:
    """B independent frames (sequences) resident in HBM for the fused finder + aligner kernel"""

    def __init__(self, device, batch, fixed_stride, moving_stride, with_prior=False):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.fixed_stride, self.moving_stride = int(batch), int(fixed_stride), int(moving_stride)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.fixed = z((batch, fixed_stride, 4), torch.float32)
        self.fixed_desc = z((batch, fixed_stride, 32), torch.uint8)
        self.n_fixed = z((batch,), torch.int32)
        self.moving = z((batch, moving_stride, 4), torch.float32)
        self.moving_desc = z((batch, moving_stride, 32), torch.uint8)
        self.n_moving = z((batch,), torch.int32)
        self.inputs_changed = torch.ones((batch,), dtype=torch.uint8, device=dev)
        self.state = z((batch, C.sizeof(PcfState)), torch.uint8)
        self.X = z((batch, 16), torch.float32)
        self.corr = z((batch, fixed_stride, 3), torch.int32)
        self.n_corr = z((batch,), torch.int32)
        self.result = z((batch, C.sizeof(AlignResult)), torch.uint8)
        self.prior = z((batch, 42), torch.float32) if with_prior else None
        self.prior_mean = None  # optional [batch, 16] float32 device tensor: mean of the motion prior
        self.max_fixed = 0  # 0 = fixed_stride; smaller bound = less LDS per frame = more frames per CU
        self.reset_state()

    def reset_state(self):
        """fresh finder objects: zeroed dynamic thresholds, config_changed = 1, identity transforms"""
        import torch
        st = PcfState()
        st.config_changed = 1
        for i in (0, 5, 10, 15):
            st.local_map_in_sensor[i] = 1.0
            st.local_map_in_sensor_previous[i] = 1.0
        raw = np.frombuffer(bytes(st), dtype=np.uint8)
        self.state[:] = torch.from_numpy(raw.copy()).to(self.state.device)
        self.n_corr.zero_()

    def upload(self, b, fixed, fixed_desc, moving_xyz, info_scale, moving_desc, X_init):
        import torch
        fixed = np.ascontiguousarray(fixed, dtype=np.float32)
        nf, nm = fixed.shape[0], len(moving_xyz)
        f4 = np.zeros((nf, 4), dtype=np.float32)
        f4[:, : fixed.shape[1]] = fixed
        m4 = np.ones((nm, 4), dtype=np.float32)
        m4[:, :3] = moving_xyz
        if info_scale is not None:
            m4[:, 3] = info_scale
        if nf:
            self.fixed[b, :nf] = torch.from_numpy(f4)
            self.fixed_desc[b, :nf] = torch.from_numpy(np.ascontiguousarray(fixed_desc, dtype=np.uint8))
        if nm:
            self.moving[b, :nm] = torch.from_numpy(m4)
            self.moving_desc[b, :nm] = torch.from_numpy(np.ascontiguousarray(moving_desc, dtype=np.uint8))
        self.n_fixed[b] = nf
        self.n_moving[b] = nm
        self.X[b] = torch.from_numpy(np.ascontiguousarray(X_init, dtype=np.float32).reshape(16))

    def descriptor(self):
        d = AlignBatch()
        d.batch, d.fixed_stride, d.moving_stride = self.batch, self.fixed_stride, self.moving_stride
        d.fixed, d.fixed_desc, d.n_fixed = self.fixed.data_ptr(), self.fixed_desc.data_ptr(), self.n_fixed.data_ptr()
        d.moving, d.moving_desc, d.n_moving = self.moving.data_ptr(), self.moving_desc.data_ptr(), self.n_moving.data_ptr()
        d.inputs_changed, d.state, d.X = self.inputs_changed.data_ptr(), self.state.data_ptr(), self.X.data_ptr()
        d.corr, d.n_corr, d.result = self.corr.data_ptr(), self.n_corr.data_ptr(), self.result.data_ptr()
        d.prior = self.prior.data_ptr() if self.prior is not None else None
        d.prior_mean = self.prior_mean.data_ptr() if self.prior_mean is not None else None
        d.max_fixed = int(self.max_fixed)
        return d

    def result_of(self, b):
        raw = self.result[b].cpu().numpy().tobytes()
        return AlignResult.from_buffer_copy(raw)

    def state_of(self, b):
        raw = self.state[b].cpu().numpy().tobytes()
        return PcfState.from_buffer_copy(raw)

    def corr_of(self, b):
        n = int(self.n_corr[b].item())
        raw = self.corr[b, :n].cpu().numpy()
        out = np.zeros(n, dtype=CORR_DTYPE)
        out["fixed_idx"], out["moving_idx"] = raw[:, 0], raw[:, 1]
        out["response"] = raw[:, 2].view(np.float32)
        return out


def align_batch(ctx, finder_params, aligner_params_, frames, mode=_lib.MODE_ALIGN):
    """prs_align_batch_run: the finder + aligner loop of every frame of the batch (mode ALIGN blocks until it is complete)"""
    d = frames.descriptor()
    return _run(ctx, "prs_align_batch_run", C.byref(finder_params), C.byref(aligner_params_), C.byref(d), int(mode))


def align_batch_enqueue(ctx, finder_params, aligner_params_, frames, rounds=0):
    """prs_align_batch_enqueue: `rounds` search + Gauss-Newton rounds on the context stream, no host synchronisation"""
    d = frames.descriptor()
    return _run(ctx, "prs_align_batch_enqueue", C.byref(finder_params), C.byref(aligner_params_), C.byref(d), int(rounds))


def align_batch_finish(ctx):
    """prs_align_batch_finish: wait for the enqueued batch, run more rounds for frames that are still pending"""
    return _run(ctx, "prs_align_batch_finish")


def align_batch_rearm(ctx, replay_stream=None):
    """prs_align_batch_rearm{,_on}: after replaying a HIP graph captured around align_batch_enqueue, so that finish checks the replay
    (replay_stream: the hipStream_t handle the graph was launched on when that is not the capture stream)"""
    if replay_stream is None:
        rc = _lib.load().prs_align_batch_rearm(ctx._h)
    else:
        rc = _lib.load().prs_align_batch_rearm_on(ctx._h, C.c_void_p(int(replay_stream)))
    _check(ctx, rc, "prs_align_batch_rearm")
    return rc


# ---- scene clipper (SceneClipperProjective3D, mapping/scene_clipper_projective_3d.cpp:9-67) ----
def projector_params(cfg):
    """prs_projector from a config's camera + projector section"""
    return pcf_params(cfg).projector


def scene_clip(ctx, projector, robot_in_local_map, sensor_in_robot, scene_xyzw, scene_desc=None):
    """host arrays, one scene -> (clipped_xyzw [m,4], clipped_desc [m,32] | None, global_indices [m], warning bits)"""
    xyzw = _np(scene_xyzw, np.float32, (-1, 4))
    n = xyzw.shape[0]
    desc = None if scene_desc is None else _np(scene_desc, np.uint8, (-1, 32))
    R = _np(robot_in_local_map, np.float32, (16,))
    S = _np(sensor_in_robot, np.float32, (16,))
    out_xyzw = np.zeros((max(n, 1), 4), dtype=np.float32)
    out_desc = None if desc is None else np.zeros((max(n, 1), 32), dtype=np.uint8)
    out_idx = np.zeros(max(n, 1), dtype=np.int32)
    m = C.c_int32(0)
    rc = _lib.load().prs_scene_clip(ctx._h, C.byref(projector), _p(R), _p(S), _p(xyzw), None if desc is None else _p(desc), n,
                                    _p(out_xyzw), None if out_desc is None else _p(out_desc), _p(out_idx), out_idx.shape[0], C.byref(m))
    _check(ctx, rc, "prs_scene_clip")
    k = m.value
    return out_xyzw[:k].copy(), (None if out_desc is None else out_desc[:k].copy()), out_idx[:k].copy(), rc


class ClipScenes:
    """B local maps resident in HBM + the clipper's outputs (laid out like the aligner's moving cloud)"""

    def __init__(self, device, batch, stride, with_desc=True):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.stride = int(batch), int(stride)
        self.scene_xyzw = torch.zeros((batch, stride, 4), dtype=torch.float32, device=dev)
        self.scene_desc = torch.zeros((batch, stride, 32), dtype=torch.uint8, device=dev) if with_desc else None
        self.n_scene = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.robot_in_local_map = torch.eye(4, dtype=torch.float32, device=dev).repeat(batch, 1, 1).contiguous()
        self.clipped_xyzw = torch.zeros((batch, stride, 4), dtype=torch.float32, device=dev)
        self.clipped_desc = torch.zeros((batch, stride, 32), dtype=torch.uint8, device=dev) if with_desc else None
        self.global_indices = torch.zeros((batch, stride), dtype=torch.int32, device=dev)
        self.n_clipped = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((batch,), dtype=torch.int32, device=dev)

    def upload(self, b, xyzw, desc, robot_in_local_map):
        import torch
        n = len(xyzw)
        dev = self.scene_xyzw.device
        if n:
            self.scene_xyzw[b, :n] = torch.from_numpy(np.ascontiguousarray(xyzw, dtype=np.float32).reshape(n, 4)).to(dev)
            if self.scene_desc is not None:
                self.scene_desc[b, :n] = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.uint8).reshape(n, 32)).to(dev)
        self.n_scene[b] = n
        self.robot_in_local_map[b] = torch.from_numpy(np.ascontiguousarray(robot_in_local_map, dtype=np.float32).reshape(4, 4)).to(dev)

    def descriptor(self):
        d = _lib.ClipBatch()
        d.batch, d.stride = self.batch, self.stride
        d.scene_xyzw = self.scene_xyzw.data_ptr()
        d.scene_desc = self.scene_desc.data_ptr() if self.scene_desc is not None else None
        d.n_scene = self.n_scene.data_ptr()
        d.robot_in_local_map = self.robot_in_local_map.data_ptr()
        d.clipped_xyzw = self.clipped_xyzw.data_ptr()
        d.clipped_desc = self.clipped_desc.data_ptr() if self.clipped_desc is not None else None
        d.global_indices = self.global_indices.data_ptr()
        d.n_clipped = self.n_clipped.data_ptr()
        d.status = self.status.data_ptr()
        d.scene_n_opt = self.scene_n_opt.data_ptr() if getattr(self, "scene_n_opt", None) is not None else None
        return d

    def clipped_of(self, b):
        m = int(self.n_clipped[b].item())
        return (self.clipped_xyzw[b, :m].cpu().numpy(),
                None if self.clipped_desc is None else self.clipped_desc[b, :m].cpu().numpy(),
                self.global_indices[b, :m].cpu().numpy(), int(self.status[b].item()))


def scene_clip_batch(ctx, projector, sensor_in_robot, scenes):
    """enqueue the clipper for every scene of the batch on the context stream (asynchronous)"""
    S = _np(sensor_in_robot, np.float32, (16,))
    d = scenes.descriptor()
    return _run(ctx, "prs_scene_clip_batch", C.byref(projector), _p(S), C.byref(d))


# ---- bijective brute-force matcher (CF/correspondence_finder_descriptor_based_bruteforce_impl.cpp) ----
def bruteforce_params(maximum_descriptor_distance=50.0, maximum_distance_ratio_to_second_best=0.9, minimum_matching_ratio=0.25):
    """defaults of CF/correspondence_finder_descriptor_based_bruteforce.h:22-36"""
    return _lib.BruteforceParams(maximum_descriptor_distance, maximum_distance_ratio_to_second_best, minimum_matching_ratio)


def bruteforce_match(ctx, params, desc_fixed, desc_moving):
    """host arrays, one pair of clouds -> (correspondences [CORR_DTYPE] ordered by (response, fixed), warning bits)"""
    df, dm = _np(desc_fixed, np.uint8, (-1, 32)), _np(desc_moving, np.uint8, (-1, 32))
    nf, nm = df.shape[0], dm.shape[0]
    out = np.zeros(max(min(nf, nm), 1), dtype=CORR_DTYPE)
    n = C.c_int32(0)
    rc = _lib.load().prs_bruteforce_match(ctx._h, C.byref(params), _p(df), nf, _p(dm), nm, _p(out), out.shape[0], C.byref(n))
    _check(ctx, rc, "prs_bruteforce_match")
    return out[: n.value].copy(), rc


class BruteforceClouds:
    """B (fixed, moving) descriptor cloud pairs resident in HBM + the matcher's outputs"""

    def __init__(self, device, batch, fixed_stride, moving_stride, candidate_capacity=0):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.fixed_stride, self.moving_stride = int(batch), int(fixed_stride), int(moving_stride)
        self.candidate_capacity = int(candidate_capacity)
        self.fixed_desc = torch.zeros((batch, fixed_stride, 32), dtype=torch.uint8, device=dev)
        self.moving_desc = torch.zeros((batch, moving_stride, 32), dtype=torch.uint8, device=dev)
        self.n_fixed = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.n_moving = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.out_stride = min(self.fixed_stride, self.moving_stride)
        self.matches = torch.zeros((batch, self.out_stride, 3), dtype=torch.int32, device=dev)
        self.n_matches = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((batch,), dtype=torch.int32, device=dev)

    def upload(self, b, desc_fixed, desc_moving):
        import torch
        dev = self.fixed_desc.device
        nf, nm = len(desc_fixed), len(desc_moving)
        if nf:
            self.fixed_desc[b, :nf] = torch.from_numpy(np.ascontiguousarray(desc_fixed, dtype=np.uint8).reshape(nf, 32)).to(dev)
        if nm:
            self.moving_desc[b, :nm] = torch.from_numpy(np.ascontiguousarray(desc_moving, dtype=np.uint8).reshape(nm, 32)).to(dev)
        self.n_fixed[b], self.n_moving[b] = nf, nm

    def descriptor(self):
        d = _lib.BruteforceBatch()
        d.batch, d.fixed_stride, d.moving_stride = self.batch, self.fixed_stride, self.moving_stride
        d.fixed_desc, d.n_fixed = self.fixed_desc.data_ptr(), self.n_fixed.data_ptr()
        d.moving_desc, d.n_moving = self.moving_desc.data_ptr(), self.n_moving.data_ptr()
        d.matches, d.n_matches, d.status = self.matches.data_ptr(), self.n_matches.data_ptr(), self.status.data_ptr()
        d.candidate_capacity = self.candidate_capacity
        return d

    def matches_of(self, b):
        n = int(self.n_matches[b].item())
        raw = self.matches[b, :n].cpu().numpy()
        out = np.zeros(n, dtype=CORR_DTYPE)
        out["fixed_idx"], out["moving_idx"] = raw[:, 0], raw[:, 1]
        out["response"] = raw[:, 2].view(np.float32)
        return out


def bruteforce_match_batch(ctx, params, clouds):
    """enqueue the matcher for every cloud pair of the batch on the context stream (asynchronous)"""
    d = clouds.descriptor()
    return _run(ctx, "prs_bruteforce_match_batch", C.byref(params), C.byref(d))


# ---- loop aligner (MultiAligner3DQR "loop_aligner" + AlignerSliceProcessor3D, registration/aligner_slice_processor_3d.hpp:7-22) ----
def point_align_params(loop, linearize_only=0, parked_per_lane=0, **overrides):
    """prs_point_align_params from a configs.py `loop` group (the loop detector's verdict thresholds); overrides by field name"""
    p = _lib.PointAlignParams()
    p.robustifier = _lib.ROBUSTIFIER_SATURATED if loop["robustifier"] == "saturated" else _lib.ROBUSTIFIER_CLAMP
    p.chi_threshold, p.damping = loop["chi_threshold"], loop["damping"]
    p.max_iterations, p.min_num_inliers = loop["max_iterations"], loop["min_num_inliers"]
    p.min_num_correspondences = loop["min_num_correspondences"]
    p.relocalize_min_inliers = loop["relocalize_min_inliers"]
    p.relocalize_min_inliers_ratio = loop["relocalize_min_inliers_ratio"]
    p.relocalize_max_chi_inliers = loop["relocalize_max_chi_inliers"]
    p.linearize_only, p.parked_per_lane = int(linearize_only), int(parked_per_lane)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _result_dict(r):
    return dict(H=np.ctypeslib.as_array(r.H).reshape(6, 6).copy(), b=np.ctypeslib.as_array(r.b).copy(), chi_inliers=np.float32(r.chi_inliers),
                chi_total=np.float32(r.chi_total), num_inliers=r.num_inliers, num_outliers=r.num_outliers, num_invalid=r.num_invalid,
                num_correspondences=r.num_correspondences, status=r.status, accepted=r.accepted, iterations=r.iterations, warnings=r.warnings)


def point_align(ctx, params, fixed_xyz, moving_xyz, corr, X_init, with_mask=True):
    """host arrays, one pair -> (X [4, 4], result dict, inlier mask [n] | None, status).  corr: CORR_DTYPE or [n, 2] (fixed, moving)"""
    f, m = _np(fixed_xyz, np.float32, (-1, 3)), _np(moving_xyz, np.float32, (-1, 3))
    c = _corr_rows(corr)
    X = _np(X_init, np.float32, (4, 4)).copy()
    res = _lib.PointAlignResult()
    mask = np.zeros(max(len(c), 1), np.uint8) if with_mask else None
    rc = _lib.load().prs_point_align(ctx._h, C.byref(params), _p(f), f.shape[0], _p(m), m.shape[0], _p(c), len(c), _p(X), C.byref(res),
                                     _p(mask) if with_mask else None)
    _check(ctx, rc, "prs_point_align")
    return X, _result_dict(res), (mask[: len(c)].copy() if with_mask else None), rc


def _corr_rows(corr):
    corr = np.asarray(corr)
    out = np.zeros(len(corr), dtype=CORR_DTYPE)
    if len(corr):
        if corr.dtype.names:
            out["fixed_idx"], out["moving_idx"] = corr["fixed_idx"], corr["moving_idx"]
        else:
            out["fixed_idx"], out["moving_idx"] = corr[:, 0], corr[:, 1]
    return out


class PointAlignBatch:
    """B (fixed, moving) point-cloud pairs resident in HBM, their correspondences, estimates and results.  `corr`, `n_corr` and
    `match_status` may be another batch's tensors (LoopClosureBatch points them at the brute-force matcher's outputs)."""

    def __init__(self, device, batch, fixed_stride, moving_stride, corr_stride=None, with_mask=True, with_status=False, corr=None,
                 n_corr=None, match_status=None):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.fixed_stride, self.moving_stride = int(batch), int(fixed_stride), int(moving_stride)
        self.corr_stride = int(corr_stride if corr_stride is not None else min(fixed_stride, moving_stride))
        self.fixed = torch.zeros((batch, fixed_stride, 4), dtype=torch.float32, device=dev)
        self.moving = torch.zeros((batch, moving_stride, 4), dtype=torch.float32, device=dev)
        self.n_fixed = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.n_moving = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.corr = corr if corr is not None else torch.zeros((batch, self.corr_stride, 3), dtype=torch.int32, device=dev)
        self.n_corr = n_corr if n_corr is not None else torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.match_status = match_status if match_status is not None else (
            torch.zeros((batch,), dtype=torch.int32, device=dev) if with_status else None)
        self.X = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(batch, 1).contiguous()
        self.result = torch.zeros((batch, C.sizeof(_lib.PointAlignResult) // 4), dtype=torch.int32, device=dev)
        self.inlier_mask = torch.zeros((batch, self.corr_stride), dtype=torch.uint8, device=dev) if with_mask else None

    def upload(self, b, fixed_xyz, moving_xyz, corr=None, X_init=None):
        import torch
        dev = self.fixed.device
        f, m = _np(fixed_xyz, np.float32, (-1, 3)), _np(moving_xyz, np.float32, (-1, 3))
        if len(f):
            self.fixed[b, : len(f), :3] = torch.from_numpy(f).to(dev)
        if len(m):
            self.moving[b, : len(m), :3] = torch.from_numpy(m).to(dev)
        self.n_fixed[b], self.n_moving[b] = len(f), len(m)
        if corr is not None:
            c = _corr_rows(corr)
            if len(c):
                self.corr[b, : len(c)] = torch.from_numpy(c.view(np.int32).reshape(-1, 3).copy()).to(dev)
            self.n_corr[b] = len(c)
        self.X[b] = torch.from_numpy(_np(np.eye(4) if X_init is None else X_init, np.float32, (16,))).to(dev)

    def descriptor(self):
        d = _lib.PointAlignPairs()
        d.batch, d.fixed_stride, d.moving_stride, d.corr_stride = self.batch, self.fixed_stride, self.moving_stride, self.corr_stride
        d.fixed, d.n_fixed, d.moving, d.n_moving = self.fixed.data_ptr(), self.n_fixed.data_ptr(), self.moving.data_ptr(), self.n_moving.data_ptr()
        d.corr, d.n_corr = self.corr.data_ptr(), self.n_corr.data_ptr()
        d.match_status = self.match_status.data_ptr() if self.match_status is not None else None
        d.X, d.result = self.X.data_ptr(), self.result.data_ptr()
        d.inlier_mask = self.inlier_mask.data_ptr() if self.inlier_mask is not None else None
        return d

    def X_of(self, b):
        return self.X[b].cpu().numpy().reshape(4, 4).copy()

    def result_of(self, b):
        raw = self.result[b].cpu().numpy().copy()
        return _result_dict(_lib.PointAlignResult.from_buffer_copy(raw.tobytes()))

    def mask_of(self, b):
        n = int(self.n_corr[b].item())
        return self.inlier_mask[b, : max(n, 0)].cpu().numpy().copy()


def point_align_batch(ctx, params, pairs):
    """enqueue the loop aligner for every pair of the batch on the context stream (asynchronous)"""
    d = pairs.descriptor()
    return _run(ctx, "prs_point_align_batch", C.byref(params), C.byref(d))


class LoopClosureBatch:
    """descriptors -> brute-force matches -> registered pose and verdict for B (query, reference) pairs, device-resident: the
    matcher's correspondences, counts and status words feed the aligner directly (fixed = query, moving = reference), both
    enqueued back to back on the context stream with no host round trip."""

    def __init__(self, device, batch, fixed_stride, moving_stride, with_mask=True, candidate_capacity=0):
        self.clouds = BruteforceClouds(device, batch, fixed_stride, moving_stride, candidate_capacity)
        self.pairs = PointAlignBatch(device, batch, fixed_stride, moving_stride, corr_stride=self.clouds.out_stride, with_mask=with_mask,
                                     corr=self.clouds.matches, n_corr=self.clouds.n_matches, match_status=self.clouds.status)

    def upload(self, b, fixed_xyz, fixed_desc, moving_xyz, moving_desc, X_init=None):
        self.clouds.upload(b, fixed_desc, moving_desc)
        self.pairs.upload(b, fixed_xyz, moving_xyz, None, X_init)

    def run(self, ctx, matcher_params, align_params):
        bruteforce_match_batch(ctx, matcher_params, self.clouds)
        return point_align_batch(ctx, align_params, self.pairs)


# ---- loop detector: place database + candidate search (CorrespondenceFinderHBST_, correspondence_finder_hbst.cpp:5-127) ----
def place_params(place, max_candidates=8, **overrides):
    """prs_place_params from a configs.py `place` group; overrides by field name"""
    p = _lib.PlaceParams()
    p.maximum_descriptor_distance = place["maximum_descriptor_distance"]
    p.minimum_age_difference_to_candidates = place["minimum_age_difference_to_candidates"]
    p.relocalize_min_inliers = place["relocalize_min_inliers"]
    p.max_candidates = int(max_candidates)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


class PlaceDatabase:
    """prs_place_db: the descriptors (and points) of every earlier local map, resident in HBM"""

    def __init__(self, ctx):
        self._ctx = ctx
        h = C.c_void_p()
        _check(ctx, _lib.load().prs_place_db_create(ctx._h, C.byref(h)), "prs_place_db_create")
        self._h = h
        ctx._children.add(self)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().prs_place_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, graph_id, desc, xyz=None, valid=None):
        """addPreviousQuery: store a local map (its Valid descriptors and points) as the next map index"""
        d = _np(desc, np.uint8, (-1, 32))
        x = _np(xyz, np.float32, (-1, 3)) if xyz is not None else None
        v = _np(valid, np.uint8, (-1,)) if valid is not None else None
        rc = _lib.load().prs_place_db_add(self._h, int(graph_id), _p(x) if x is not None else None, _p(d), _p(v) if v is not None else None,
                                          d.shape[0])
        return _check(self._ctx, rc, "prs_place_db_add")

    def clear(self):
        _check(self._ctx, _lib.load().prs_place_db_clear(self._h), "prs_place_db_clear")

    def reserve(self, maps, rows):
        _check(self._ctx, _lib.load().prs_place_db_reserve(self._h, int(maps), int(rows)), "prs_place_db_reserve")

    def size(self):
        """(maps, rows with pads, largest map)"""
        m, r, x = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(self._ctx, _lib.load().prs_place_db_size(self._h, C.byref(m), C.byref(r), C.byref(x)), "prs_place_db_size")
        return m.value, r.value, x.value

    def query(self, params, graph_id, desc, valid=None, corr_stride=None):
        """host arrays, one query -> dict(status, candidates, corr [list of CORR_DTYPE], counts [maps])"""
        maps, _, big = self.size()
        d = _np(desc, np.uint8, (-1, 32))
        v = _np(valid, np.uint8, (-1,)) if valid is not None else None
        k = params.max_candidates
        stride = max(int(corr_stride if corr_stride is not None else big), 1)
        cand = np.zeros(max(k, 1), np.int32)
        ncorr = np.zeros(max(k, 1), np.int32)
        corr = np.zeros(max(k, 1) * stride, CORR_DTYPE)
        counts = np.zeros(max(maps, 1), np.uint32)
        nc = C.c_int32(0)
        rc = _lib.load().prs_place_query(self._h, C.byref(params), int(graph_id), _p(d), _p(v) if v is not None else None, d.shape[0],
                                         _p(cand), C.byref(nc), _p(corr), stride, _p(ncorr), _p(counts))
        _check(self._ctx, rc, "prs_place_query")
        n = nc.value
        return dict(status=rc, candidates=cand[:n].tolist(), counts=counts[:maps].astype(np.int64),
                    corr=[corr[i * stride: i * stride + ncorr[i]].copy() for i in range(n)])


class PlaceQueries:
    """B queries resident in HBM and the candidate search's outputs, sized for `db` as it stands (count / key / corr strides)"""

    def __init__(self, device, batch, query_stride, max_candidates, db=None, count_stride=None, key_stride=None, corr_stride=None,
                 with_valid=False):
        import torch
        dev = torch.device("cuda", device)
        maps, rows, big = db.size() if db is not None else (0, 0, 0)
        self.batch, self.query_stride, self.max_candidates = int(batch), int(query_stride), int(max_candidates)
        self.count_stride = max(int(count_stride if count_stride is not None else maps), 1)
        self.key_stride = max(int(key_stride if key_stride is not None else rows), 1)
        self.corr_stride = max(int(corr_stride if corr_stride is not None else big), 1)
        self.desc = torch.zeros((batch, query_stride, 32), dtype=torch.uint8, device=dev)
        self.valid = torch.ones((batch, query_stride), dtype=torch.uint8, device=dev) if with_valid else None
        self.xyz = torch.zeros((batch, query_stride, 4), dtype=torch.float32, device=dev)
        self.n_query = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.graph_id = torch.zeros((batch,), dtype=torch.int64, device=dev)
        self.match_counts = torch.zeros((batch, self.count_stride), dtype=torch.int32, device=dev)
        self.best_keys = torch.zeros((batch, self.key_stride), dtype=torch.int32, device=dev)
        self.candidates = torch.zeros((batch, max_candidates), dtype=torch.int32, device=dev)
        self.n_candidates = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.corr = torch.zeros((batch, max_candidates, self.corr_stride, 3), dtype=torch.int32, device=dev)
        self.n_corr = torch.zeros((batch, max_candidates), dtype=torch.int32, device=dev)
        self.status = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.index_query = torch.zeros((batch,), dtype=torch.int64, device=dev)

    def upload(self, b, graph_id, desc, xyz=None, valid=None):
        import torch
        dev = self.desc.device
        d = _np(desc, np.uint8, (-1, 32))
        n = d.shape[0]
        if n:
            self.desc[b, :n] = torch.from_numpy(d).to(dev)
            if xyz is not None:
                self.xyz[b, :n, :3] = torch.from_numpy(_np(xyz, np.float32, (-1, 3))).to(dev)
        if valid is not None:
            self.valid[b, :n] = torch.from_numpy(_np(valid, np.uint8, (-1,))).to(dev)
        self.n_query[b], self.graph_id[b] = n, int(graph_id)

    def descriptor(self):
        d = _lib.PlaceQueries()
        d.batch, d.query_stride = self.batch, self.query_stride
        d.desc, d.xyz, d.n_query, d.graph_id = self.desc.data_ptr(), self.xyz.data_ptr(), self.n_query.data_ptr(), self.graph_id.data_ptr()
        d.valid = self.valid.data_ptr() if self.valid is not None else None
        d.count_stride, d.match_counts = self.count_stride, self.match_counts.data_ptr()
        d.key_stride, d.best_keys = self.key_stride, self.best_keys.data_ptr()
        d.corr_stride, d.candidates, d.n_candidates = self.corr_stride, self.candidates.data_ptr(), self.n_candidates.data_ptr()
        d.corr, d.n_corr, d.status, d.index_query = self.corr.data_ptr(), self.n_corr.data_ptr(), self.status.data_ptr(), self.index_query.data_ptr()
        return d

    def result_of(self, b, maps=None):
        """dict(status, index_query, candidates, corr [list of CORR_DTYPE], counts [maps])"""
        n = int(self.n_candidates[b].item())
        corr = []
        for k in range(n):
            m = int(self.n_corr[b, k].item())
            raw = self.corr[b, k, :m].cpu().numpy()
            c = np.zeros(m, CORR_DTYPE)
            c["fixed_idx"], c["moving_idx"], c["response"] = raw[:, 0], raw[:, 1], raw[:, 2].view(np.float32)
            corr.append(c)
        counts = self.match_counts[b].cpu().numpy().view(np.uint32).astype(np.int64)
        return dict(status=int(self.status[b].item()), index_query=int(self.index_query[b].item()),
                    candidates=self.candidates[b, :n].cpu().numpy().tolist(), corr=corr,
                    counts=counts[: maps] if maps is not None else counts)


def place_query_batch(ctx, db, params, queries):
    """enqueue the candidate search for every query of the batch on the context stream (asynchronous)"""
    d = queries.descriptor()
    rc = _lib.load().prs_place_query_batch(db._h, C.byref(params), C.byref(d))
    _check(ctx, rc, "prs_place_query_batch")
    return rc


class LoopDetectorBatch:
    """B query local maps -> candidate search -> one loop-closure pair slot per (query, candidate) -> brute-force matcher -> loop
    aligner and verdict, all enqueued on the context stream with no host round trip.  Slot b * max_candidates + k holds query b
    against its k-th candidate; slots without a candidate carry n = 0 and are never accepted."""

    def __init__(self, device, db, batch, query_stride, max_candidates, moving_stride=None, with_valid=False, candidate_capacity=None):
        _, _, big = db.size()
        self.db, self.batch, self.max_candidates = db, int(batch), int(max_candidates)
        self.queries = PlaceQueries(device, batch, query_stride, max_candidates, db, with_valid=with_valid)
        ms = max(int(moving_stride if moving_stride is not None else big), 1)
        slots = self.batch * self.max_candidates
        # the matcher's candidate list per slot: by default room for every pair (0 = the matcher's own default, 16 x the larger cloud)
        cap = query_stride * ms if candidate_capacity is None else int(candidate_capacity)
        self.closures = LoopClosureBatch(device, slots, query_stride, ms, with_mask=False, candidate_capacity=cap)
        # one set of point counts per slot: the gather writes the matcher's, the aligner reads the same tensors
        self.closures.pairs.n_fixed, self.closures.pairs.n_moving = self.closures.clouds.n_fixed, self.closures.clouds.n_moving

    def upload(self, b, graph_id, desc, xyz, valid=None):
        self.queries.upload(b, graph_id, desc, xyz, valid)

    def pairs_descriptor(self):
        lc = self.closures
        d = _lib.PlacePairs()
        d.fixed_stride, d.moving_stride = lc.pairs.fixed_stride, lc.pairs.moving_stride
        d.fixed_xyz, d.fixed_desc, d.n_fixed = lc.pairs.fixed.data_ptr(), lc.clouds.fixed_desc.data_ptr(), lc.clouds.n_fixed.data_ptr()
        d.moving_xyz, d.moving_desc, d.n_moving = lc.pairs.moving.data_ptr(), lc.clouds.moving_desc.data_ptr(), lc.clouds.n_moving.data_ptr()
        d.X = lc.pairs.X.data_ptr()
        return d

    def run(self, ctx, place_params_, matcher_params, align_params):
        place_query_batch(ctx, self.db, place_params_, self.queries)
        q, pairs = self.queries.descriptor(), self.pairs_descriptor()
        _check(ctx, _lib.load().prs_place_gather_pairs(self.db._h, C.byref(place_params_), C.byref(q), C.byref(pairs)), "prs_place_gather_pairs")
        lc = self.closures
        # the aligner's point counts are the matcher's (one cloud pair per slot)
        bruteforce_match_batch(ctx, matcher_params, lc.clouds)
        return point_align_batch(ctx, align_params, lc.pairs)

    def result_of(self, b):
        """dict(candidates, poses [4, 4] per candidate, accepted per candidate, search result)"""
        r = self.queries.result_of(b, self.db.size()[0])
        slots = [b * self.max_candidates + k for k in range(len(r["candidates"]))]
        return dict(candidates=r["candidates"], poses=[self.closures.pairs.X_of(s) for s in slots],
                    accepted=[self.closures.pairs.result_of(s)["accepted"] for s in slots], search=r)


# ---- place bank: one place database per sequence, contents and sizes on the device (include/proslam_hip.h prs_place_bank_*) ----
class PlaceBank:
    """prs_place_bank: `batch` independent place databases in fixed device arenas (map_stride maps, row_stride rows each).  Maps are
    stored by a kernel (append) and the sizes are device counters, so a captured step sees what earlier replays stored."""

    def __init__(self, ctx, batch, map_stride, row_stride):
        import torch
        self._ctx = ctx
        h = C.c_void_p()
        _check(ctx, _lib.load().prs_place_bank_create(ctx._h, int(batch), int(map_stride), int(row_stride), C.byref(h)), "prs_place_bank_create")
        self._h = h
        ctx._children.add(self)
        self.batch, self.map_stride, self.row_stride = int(batch), int(map_stride), (int(row_stride) + 15) // 16 * 16
        dev = torch.device("cuda", ctx.device)
        # node_of_map lives in a tensor, so that PoseGraphBatch.append_closures reads it in place
        self.node_of_map = torch.full((self.batch, self.map_stride), -1, dtype=torch.int32, device=dev)
        _check(ctx, _lib.load().prs_place_bank_bind_node_of_map(self._h, self.node_of_map.data_ptr()), "prs_place_bank_bind_node_of_map")
        self.append_status = torch.zeros((self.batch,), dtype=torch.int32, device=dev)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().prs_place_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, queries, graph_id_base=None):
        """enqueue addPreviousQuery for every sequence: slot b of `queries` (a PlaceQueries, or anything with its batch,
        query_stride, desc, xyz, valid, n_query and graph_id) becomes the next map of database b; n_query == 0 stores nothing.
        graph_id_base: int64 device tensor [batch] or None.  Per-sequence status lands in self.append_status (asynchronous)."""
        a = _lib.PlaceBankAppend()
        a.batch, a.query_stride = int(queries.batch), int(queries.query_stride)
        a.desc, a.n_query, a.graph_id = queries.desc.data_ptr(), queries.n_query.data_ptr(), queries.graph_id.data_ptr()
        xyz, valid = getattr(queries, "xyz", None), getattr(queries, "valid", None)
        a.xyz = xyz.data_ptr() if xyz is not None else None
        a.valid = valid.data_ptr() if valid is not None else None
        a.graph_id_base = graph_id_base.data_ptr() if graph_id_base is not None else None
        a.status = self.append_status.data_ptr()
        self._append_keep = (queries, graph_id_base)  # alive until the kernel has run
        return _check(self._ctx, _lib.load().prs_place_bank_append_batch(self._h, C.byref(a)), "prs_place_bank_append_batch")

    def clear(self):
        _check(self._ctx, _lib.load().prs_place_bank_clear(self._h), "prs_place_bank_clear")

    def sizes(self):
        """(maps [batch], rows with pads [batch], largest map [batch]) as int32 arrays; synchronises: tests and tools only"""
        out = [np.zeros(self.batch, np.int32) for _ in range(3)]
        _check(self._ctx, _lib.load().prs_place_bank_sizes(self._h, *(_p(o) for o in out)), "prs_place_bank_sizes")
        return tuple(out)


class PlaceBankLinks:
    """the optional outputs of place_bank_query_batch that prs_pose_graph_append_closures reads: the flat candidate list, the
    queries' nodes and (constant) the graph of every query"""

    def __init__(self, device, batch, max_candidates, graph_id_base=None):
        import torch
        dev = torch.device("cuda", device)
        self.candidates_flat = torch.full((batch, max_candidates), -1, dtype=torch.int32, device=dev)
        self.query_node = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        self.graph_of_query = torch.arange(batch, dtype=torch.int32, device=dev)
        self.graph_id_base = graph_id_base

    def descriptor(self):
        d = _lib.PlaceBankLinks()
        d.candidates_flat, d.query_node = self.candidates_flat.data_ptr(), self.query_node.data_ptr()
        d.graph_id_base = self.graph_id_base.data_ptr() if self.graph_id_base is not None else None
        return d


def place_bank_query_batch(ctx, bank, params, queries, links=None):
    """enqueue the candidate search of query b in database b for every sequence (asynchronous, no host read)"""
    d = queries.descriptor()
    ld = links.descriptor() if links is not None else None
    rc = _lib.load().prs_place_bank_query_batch(bank._h, C.byref(params), C.byref(d), C.byref(ld) if ld is not None else None)
    _check(ctx, rc, "prs_place_bank_query_batch")
    return rc


class _ClosureView:
    """what PoseGraphBatch.append_closures reads of a detector, with the bank's flat candidate list as .queries.candidates"""

    class _Q:
        def __init__(self, candidates):
            self.candidates = candidates

    def __init__(self, det):
        self.batch, self.max_candidates, self.closures = det.batch, det.max_candidates, det.closures
        self.queries = self._Q(det.links.candidates_flat)
        self._det = det

    def node_maps(self):
        """(graph_of_query, node_of_query, node_of_map): int32 device tensors"""
        return self._det.links.graph_of_query, self._det.links.query_node, self._det.bank.node_of_map.view(-1)


class BankDetectorBatch:
    """LoopDetectorBatch over a PlaceBank: query b searches database b, the pair slots are gathered, matched and aligned, and (append)
    the query itself is stored as the next map of its sequence -- query, gather, append as the reference does, all enqueued on the
    context stream with no host round trip.  moving_stride defaults to query_stride: a stored map never exceeds the slot it came
    from.  graph_id_base: int64 device tensor [batch] (the session's) or None; node = graph id - base."""

    def __init__(self, device, bank, batch, query_stride, max_candidates, moving_stride=None, with_valid=False, candidate_capacity=None,
                 graph_id_base=None):
        self.bank, self.batch, self.max_candidates = bank, int(batch), int(max_candidates)
        self.graph_id_base = graph_id_base
        self.queries = PlaceQueries(device, batch, query_stride, max_candidates, None, count_stride=bank.map_stride,
                                    key_stride=bank.row_stride, corr_stride=min(int(query_stride), bank.row_stride), with_valid=with_valid)
        self.links = PlaceBankLinks(device, self.batch, self.max_candidates, graph_id_base)
        ms = max(int(moving_stride if moving_stride is not None else query_stride), 1)
        slots = self.batch * self.max_candidates
        cap = query_stride * ms if candidate_capacity is None else int(candidate_capacity)
        self.closures = LoopClosureBatch(device, slots, query_stride, ms, with_mask=False, candidate_capacity=cap)
        self.closures.pairs.n_fixed, self.closures.pairs.n_moving = self.closures.clouds.n_fixed, self.closures.clouds.n_moving
        self.view = _ClosureView(self)

    def upload(self, b, graph_id, desc, xyz, valid=None):
        self.queries.upload(b, graph_id, desc, xyz, valid)

    pairs_descriptor = LoopDetectorBatch.pairs_descriptor

    def run(self, ctx, place_params_, matcher_params, align_params, append=True):
        place_bank_query_batch(ctx, self.bank, place_params_, self.queries, self.links)
        q, pairs = self.queries.descriptor(), self.pairs_descriptor()
        _check(ctx, _lib.load().prs_place_bank_gather_pairs(self.bank._h, C.byref(place_params_), C.byref(q), C.byref(pairs)),
               "prs_place_bank_gather_pairs")
        lc = self.closures
        bruteforce_match_batch(ctx, matcher_params, lc.clouds)
        rc = point_align_batch(ctx, align_params, lc.pairs)
        if append:
            self.bank.append(self.queries, self.graph_id_base)
        return rc

    def node_maps(self):
        return self.view.node_maps()

    def result_of(self, b, maps=None):
        """dict(candidates [map indices of sequence b], poses, accepted, search result); maps: the number of match counts to keep"""
        r = self.queries.result_of(b, maps)
        slots = [b * self.max_candidates + k for k in range(len(r["candidates"]))]
        return dict(candidates=r["candidates"], poses=[self.closures.pairs.X_of(s) for s in slots],
                    accepted=[self.closures.pairs.result_of(s)["accepted"] for s in slots], search=r,
                    query_node=int(self.links.query_node[b].item()))


# ---- pose-graph optimiser: the global solver over SE(3) graphs with loop closures (include/proslam_hip.h) ----
def pose_graph_params(cfg_graph, closure_information=1.0, **overrides):
    """prs_pose_graph_params from a configs.py `graph` group; overrides by field name"""
    p = _lib.PoseGraphParams()
    p.damping, p.damping_form = cfg_graph["damping"], _lib.DAMPING_DIAG
    p.max_iterations, p.epsilon = cfg_graph["max_iterations"], cfg_graph["epsilon"]
    p.closure_information = closure_information
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _graph_result_dict(r):
    n = r.linearizations
    return dict(chi=np.ctypeslib.as_array(r.chi)[:n].copy(), chi_final=np.float64(r.chi_final), linearizations=n, iterations=r.iterations,
                envelope_blocks=r.envelope_blocks, status=r.status)


def pose_graph_lm_params(cfg_graph, **overrides):
    """prs_pose_graph_lm_params from a configs.py `graph` group that has an `lm` sub-dict (icl, tum); overrides by field name"""
    lm = cfg_graph["lm"]
    p = _lib.PoseGraphLmParams()
    p.user_lambda_init, p.tau, p.step_high, p.step_low = lm["user_lambda_init"], lm["tau"], lm["step_high"], lm["step_low"]
    p.lm_iterations_max, p.variable_damping = lm["lm_iterations_max"], lm["variable_damping"]
    p.max_iterations, p.epsilon = cfg_graph["max_iterations"], cfg_graph["epsilon"]
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _graph_lm_result_dict(r):
    n = r.linearizations
    rounds = sum(1 for t in r.trials if t > 0)
    return dict(chi=np.ctypeslib.as_array(r.chi)[:n].copy(), chi_final=np.float64(r.chi_final),
                lam=np.ctypeslib.as_array(r.lambda_)[:rounds].copy(), trials=[int(t) for t in r.trials[:rounds]], linearizations=n,
                iterations=r.iterations, envelope_blocks=r.envelope_blocks, status=r.status, trials_total=r.trials_total,
                rejected_not_positive_definite=r.rejected_not_positive_definite, stalled=r.stalled)


def _host_graph(poses, fixed, src, dst, Z, omega):
    X = _np(poses, np.float64, (-1, 16)).copy()
    fx = _np(fixed, np.uint8, (-1,))
    f, t = _np(src, np.int32, (-1,)), _np(dst, np.int32, (-1,))
    z = _np(Z, np.float32, (-1, 16))
    om = _np(omega, np.float32, (-1, 36)) if omega is not None else None
    return X, (X.shape[0], _p(X), _p(fx), len(f), _p(f), _p(t), _p(z), _p(om) if om is not None else None), (fx, f, t, z, om)


def pose_graph_optimize(ctx, params, poses, fixed, src, dst, Z, omega=None):
    """host arrays, one graph -> (X [n, 4, 4] float64, result dict, status).  poses [n, 4, 4] float64, fixed [n], src / dst [E], Z
    [E, 4, 4] float32, omega [E, 6, 6] float32 or None (identity).  A refused or numerically failed graph raises ProslamHipError."""
    X, args, _keep = _host_graph(poses, fixed, src, dst, Z, omega)
    res = _lib.PoseGraphResult()
    rc = _lib.load().prs_pose_graph_optimize(ctx._h, C.byref(params), *args, C.byref(res))
    _check(ctx, rc, "prs_pose_graph_optimize")
    return X.reshape(-1, 4, 4), _graph_result_dict(res), rc


def pose_graph_optimize_lm(ctx, params, poses, fixed, src, dst, Z, omega=None):
    """pose_graph_optimize with the Levenberg-Marquardt loop (params: pose_graph_lm_params); the result dict adds lam and trials
    per round, trials_total, rejected_not_positive_definite and stalled"""
    X, args, _keep = _host_graph(poses, fixed, src, dst, Z, omega)
    res = _lib.PoseGraphLmResult()
    rc = _lib.load().prs_pose_graph_optimize_lm(ctx._h, C.byref(params), *args, C.byref(res))
    _check(ctx, rc, "prs_pose_graph_optimize_lm")
    return X.reshape(-1, 4, 4), _graph_lm_result_dict(res), rc


def pose_graph_algorithm(cfg_graph, **overrides):
    """(params, batch entry, host entry) for a configs.py `graph` group by its `algorithm`: IterationAlgorithmLM (icl, tum) gets the
    LM entries, IterationAlgorithmGN the Gauss-Newton ones; any other name is an error"""
    name = cfg_graph["algorithm"]
    if name == "IterationAlgorithmLM":
        return pose_graph_lm_params(cfg_graph, **overrides), pose_graph_optimize_lm_batch, pose_graph_optimize_lm
    if name == "IterationAlgorithmGN":
        return pose_graph_params(cfg_graph, **overrides), pose_graph_optimize_batch, pose_graph_optimize
    raise ValueError("no pose-graph entry for algorithm %r" % (name,))


def pose_graph_envelope_blocks(n_nodes, src, dst):
    """6 x 6 blocks of the row envelope of a graph: the sum over nodes j of j - first(j) + 1 (first = smallest neighbour, or j)"""
    first = np.arange(int(n_nodes))
    for a, b in zip(np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)):
        lo, hi = (a, b) if a < b else (b, a)
        if 0 <= lo and hi < n_nodes and lo != hi:
            first[hi] = min(first[hi], lo)
    return int(np.sum(np.arange(int(n_nodes)) - first + 1))


class PoseGraphBatch:
    """B pose graphs resident in HBM (torch tensors own the memory): poses (float64), fixed flags, edge lists with float32
    measurements and information matrices, the envelope workspace and the results.  envelope_blocks: room per graph (default: the
    full lower triangle of node_stride nodes when that is small, else 64 blocks per node).  lm=True: the workspace also holds the
    28 doubles per node of the Levenberg-Marquardt entry (pose_graph_optimize_lm_batch), whose results land in lm_result."""

    def __init__(self, device, batch, node_stride, edge_stride, envelope_blocks=None, with_omega=True, lm=False):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.node_stride, self.edge_stride = int(batch), int(node_stride), int(edge_stride)
        full = self.node_stride * (self.node_stride + 1) // 2
        self.envelope_blocks = int(envelope_blocks if envelope_blocks is not None else min(full, 64 * self.node_stride))
        self.X = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 1, 16).repeat(batch, node_stride, 1).contiguous()
        self.fixed = torch.zeros((batch, node_stride), dtype=torch.uint8, device=dev)
        self.n_nodes = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.src = torch.zeros((batch, edge_stride), dtype=torch.int32, device=dev)
        self.dst = torch.zeros((batch, edge_stride), dtype=torch.int32, device=dev)
        self.Z = torch.zeros((batch, edge_stride, 16), dtype=torch.float32, device=dev)
        self.omega = torch.zeros((batch, edge_stride, 36), dtype=torch.float32, device=dev) if with_omega else None
        self.n_edges = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.lm = bool(lm)
        size = _lib.load().prs_pose_graph_lm_workspace_bytes if self.lm else _lib.load().prs_pose_graph_workspace_bytes
        self.workspace_bytes = int(size(self.batch, self.node_stride, self.envelope_blocks))
        self.workspace = torch.zeros((max(self.workspace_bytes // 8, 1),), dtype=torch.float64, device=dev)
        self.result = torch.zeros((batch, C.sizeof(_lib.PoseGraphResult) // 8), dtype=torch.float64, device=dev)
        self.lm_result = torch.zeros((batch, C.sizeof(_lib.PoseGraphLmResult) // 8), dtype=torch.float64, device=dev)
        self.append_status = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self.n_appended = torch.zeros((batch,), dtype=torch.int32, device=dev)

    def upload(self, b, poses, fixed, edges):
        """edges: (src [E], dst [E], Z [E, 4, 4], omega [E, 6, 6] or None = identity)"""
        import torch
        dev = self.X.device
        X = _np(poses, np.float64, (-1, 16))
        src, dst, Z = _np(edges[0], np.int32, (-1,)), _np(edges[1], np.int32, (-1,)), _np(edges[2], np.float32, (-1, 16))
        omega = edges[3] if len(edges) > 3 else None
        n, e = len(X), len(src)
        if n:
            self.X[b, :n] = torch.from_numpy(X).to(dev)
            self.fixed[b, :n] = torch.from_numpy(_np(fixed, np.uint8, (-1,))).to(dev)
        if e:
            self.src[b, :e], self.dst[b, :e] = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            self.Z[b, :e] = torch.from_numpy(Z).to(dev)
            if self.omega is not None:
                om = np.tile(np.eye(6, dtype=np.float32).reshape(1, 36), (e, 1)) if omega is None else _np(omega, np.float32, (-1, 36))
                self.omega[b, :e] = torch.from_numpy(om).to(dev)
            elif omega is not None:
                raise ValueError("this batch was built without omega (identity information only)")
        self.n_nodes[b], self.n_edges[b] = n, e

    def descriptor(self):
        d = _lib.PoseGraphs()
        d.batch, d.node_stride, d.edge_stride = self.batch, self.node_stride, self.edge_stride
        d.X, d.fixed, d.n_nodes = self.X.data_ptr(), self.fixed.data_ptr(), self.n_nodes.data_ptr()
        d.from_, d.to, d.Z, d.n_edges = self.src.data_ptr(), self.dst.data_ptr(), self.Z.data_ptr(), self.n_edges.data_ptr()
        d.omega = self.omega.data_ptr() if self.omega is not None else None
        d.workspace, d.workspace_bytes, d.result = self.workspace.data_ptr(), self.workspace_bytes, self.result.data_ptr()
        return d

    def result_of(self, b):
        raw = self.result[b].cpu().numpy().copy()
        return _graph_result_dict(_lib.PoseGraphResult.from_buffer_copy(raw.tobytes()))

    def lm_result_of(self, b):
        raw = self.lm_result[b].cpu().numpy().copy()
        return _graph_lm_result_dict(_lib.PoseGraphLmResult.from_buffer_copy(raw.tobytes()))

    def poses_of(self, b):
        n = max(int(self.n_nodes[b].item()), 0)
        return self.X[b, : min(n, self.node_stride)].cpu().numpy().reshape(-1, 4, 4).copy()

    def edges_of(self, b):
        """(src, dst, Z [E, 4, 4], omega [E, 6, 6] | None) as they stand on the device"""
        e = int(self.n_edges[b].item())
        om = self.omega[b, :e].cpu().numpy().reshape(-1, 6, 6).copy() if self.omega is not None else None
        return self.src[b, :e].cpu().numpy().copy(), self.dst[b, :e].cpu().numpy().copy(), self.Z[b, :e].cpu().numpy().reshape(-1, 4, 4).copy(), om

    def append_closures(self, ctx, detector, graph_of_query, node_of_query, node_of_map, params=None):
        """enqueue the append of `detector`'s (a LoopDetectorBatch, after run()) accepted closures: query b goes to graph
        graph_of_query[b] as an edge from node_of_query[b] to node_of_map[candidate], Z = the aligner's X.  The three maps are int32
        device tensors (or arrays, uploaded here).  Per-graph status lands in self.append_status (asynchronous)."""
        import torch
        dev = self.X.device
        as_dev = lambda a: a.to(dev, torch.int32).contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(_np(a, np.int32, (-1,))).to(dev)
        self._closure_maps = (as_dev(graph_of_query), as_dev(node_of_query), as_dev(node_of_map))  # kept alive until the kernel has run
        pairs = detector.closures.pairs
        c = _lib.PoseGraphClosures()
        c.n_queries, c.max_candidates, c.n_maps = detector.batch, detector.max_candidates, int(self._closure_maps[2].numel())
        c.candidates, c.result, c.X = detector.queries.candidates.data_ptr(), pairs.result.data_ptr(), pairs.X.data_ptr()
        c.graph_of_query, c.node_of_query, c.node_of_map = (t.data_ptr() for t in self._closure_maps)
        c.status, c.n_appended = self.append_status.data_ptr(), self.n_appended.data_ptr()
        p = params if params is not None else pose_graph_params(dict(damping=0.0, max_iterations=0, epsilon=0.0))
        d = self.descriptor()
        return _run(ctx, "prs_pose_graph_append_closures", C.byref(p), C.byref(d), C.byref(c))


def pose_graph_optimize_batch(ctx, params, graphs):
    """enqueue the optimiser for every graph of the batch on the context stream (asynchronous, one launch)"""
    d = graphs.descriptor()
    return _run(ctx, "prs_pose_graph_optimize_batch", C.byref(params), C.byref(d))


def pose_graph_optimize_lm_batch(ctx, params, graphs):
    """enqueue the Levenberg-Marquardt optimiser for every graph of the batch (asynchronous, one launch); results in
    graphs.lm_result.  A batch built without lm=True has a workspace without the 28 doubles per node: its graphs whose envelope
    no longer fits report PRS_ERR_CAPACITY."""
    d = graphs.descriptor()
    return _run(ctx, "prs_pose_graph_optimize_lm_batch", C.byref(params), C.byref(d), graphs.lm_result.data_ptr())


# ---- landmark estimators + projective mergers (mapping/mergers, mapping/landmarks) ----
EST_WEIGHTED_MEAN, EST_EKF, EST_SMOOTHER = 0, 1, 2
MERGER_STEREO_TRIANGULATION, MERGER_STEREO_EKF, MERGER_DEPTH_EKF = 0, 1, 2


class MapBatch:
    """B local maps resident in HBM (structure of arrays, torch tensors own the memory) + the
    per-frame inputs of the merger.  Row layouts follow include/proslam_hip.h prs_merge_batch."""

    MEAS_WORDS = 7    # prs_camera_measurement: 3 + 3 floats + frame index
    POSE_WORDS = 24   # prs_frame_pose: two 3x4 transforms

    def __init__(self, device, batch, capacity, max_measurements, max_frames, measurement_stride, corr_stride):
        import torch
        dev = torch.device("cuda", device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.batch, self.capacity = int(batch), int(capacity)
        self.max_measurements, self.max_frames = int(max_measurements), int(max_frames)
        self.measurement_stride, self.corr_stride = int(measurement_stride), int(corr_stride)
        self.coords = z((batch, capacity, 4), torch.float32)
        self.desc = z((batch, capacity, 32), torch.uint8)
        self.state = z((batch, capacity, 4), torch.float32)
        self.covariance = z((batch, capacity, 9), torch.float32)
        self.n_opt = z((batch, capacity), torch.int32)
        self.inlier = z((batch, capacity), torch.uint8)
        self.n_meas = z((batch, capacity), torch.int32)
        self.meas = z((batch, capacity, max(max_measurements, 1), self.MEAS_WORDS), torch.int32)
        self.poses = z((batch, max_frames, self.POSE_WORDS), torch.float32)
        self.n_points = z((batch,), torch.int32)
        self.measurement = z((batch, measurement_stride, 4), torch.float32)
        self.measurement_desc = z((batch, measurement_stride, 32), torch.uint8)
        self.n_measured = z((batch,), torch.int32)
        self.corr = z((batch, corr_stride, 3), torch.int32)
        self.n_corr = z((batch,), torch.int32)
        self.scene_index_map = None
        self.corr_from_aligner = 0
        self.measurement_in_world = torch.eye(4, dtype=torch.float32, device=dev).repeat(batch, 1, 1).contiguous()
        self.measurement_in_scene = torch.eye(4, dtype=torch.float32, device=dev).repeat(batch, 1, 1).contiguous()
        self.frame = z((batch,), torch.int32)
        self.result = z((batch, 3), torch.int32)

    def descriptor(self):
        d = _lib.MergeBatch()
        d.batch, d.capacity, d.max_measurements, d.max_frames = self.batch, self.capacity, self.max_measurements, self.max_frames
        for name in ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas", "poses", "n_points", "measurement",
                     "measurement_desc", "n_measured", "corr", "n_corr", "measurement_in_world", "measurement_in_scene", "frame", "result"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.meas = self.meas.data_ptr() if self.max_measurements > 0 else None
        d.measurement_stride, d.corr_stride = self.measurement_stride, self.corr_stride
        d.scene_index_map = self.scene_index_map.data_ptr() if self.scene_index_map is not None else None
        d.corr_from_aligner = int(self.corr_from_aligner)
        return d


def merge_batch(ctx, params, maps):
    """enqueue MergerProjective_::compute for every (map, frame) pair of the batch (asynchronous)"""
    d = maps.descriptor()
    return _run(ctx, "prs_merge_batch_run", C.byref(params), C.byref(d))


class MapHandle:
    """host-side merger object: one device-resident local map (prs_map), mirrors setScene / setMeasurement / compute of
    mapping/mergers/merger_projective.h"""

    def __init__(self, ctx, capacity, max_measurements=0, max_frames=64, max_measured=2048):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.capacity = int(capacity)
        rc = _lib.load().prs_map_create(ctx._h, int(capacity), int(max_measurements), int(max_frames), int(max_measured), C.byref(self._h))
        _check(ctx, rc, "prs_map_create")
        ctx._children.add(self)  # the handle points into the context: Context.close() closes it first

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._ctx, "_h", None):  # (a context that is gone has already released the device memory's owner)
                _lib.load().prs_map_destroy(self._h)
            self._h = C.c_void_p()

    def reserve(self, capacity):
        """grow the landmark arrays in place (every landmark keeps its state, covariance and history)"""
        _check(self._ctx, _lib.load().prs_map_reserve(self._h, int(capacity)), "prs_map_reserve")
        self.capacity = max(self.capacity, int(capacity))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        _check(self._ctx, _lib.load().prs_map_clear(self._h), "prs_map_clear")

    def size(self):
        n, f = C.c_int32(0), C.c_int32(0)
        _check(self._ctx, _lib.load().prs_map_size(self._h, C.byref(n), C.byref(f)), "prs_map_size")
        return n.value, f.value

    def set_scene(self, coords, desc, state=None, covariance=None, n_opt=None, first_measurement=None):
        c = _np(coords, np.float32, (-1, 3))
        n = c.shape[0]
        d = _np(desc, np.uint8, (-1, 32))
        st = None if state is None else _np(state, np.float32, (-1, 3))
        cov = None if covariance is None else _np(covariance, np.float32, (-1, 9))
        no = None if n_opt is None else _np(n_opt, np.uint32, (-1,))
        fm = None if first_measurement is None else np.ascontiguousarray(first_measurement)
        rc = _lib.load().prs_map_set_scene(self._h, _p(c), None if st is None else _p(st), None if cov is None else _p(cov), _p(d),
                                           None if no is None else _p(no), None if fm is None else fm.ctypes.data, n)
        _check(self._ctx, rc, "prs_map_set_scene")

    def set_frame_pose(self, frame, sensor_in_world):
        T = _np(sensor_in_world, np.float32, (16,))
        _check(self._ctx, _lib.load().prs_map_set_frame_pose(self._h, int(frame), _p(T)), "prs_map_set_frame_pose")

    def merge(self, params, measurement_in_world, measurement_in_scene, measurement, measurement_desc, corr, scene_index_map=None, corr_from_aligner=0):
        """-> (n_merged, n_added, status bits)"""
        dim = int(params.estimator.measurement_dim)
        z = _np(measurement, np.float32, (-1, dim))
        d = _np(measurement_desc, np.uint8, (-1, 32))
        c = np.ascontiguousarray(corr, dtype=CORR_DTYPE)
        im = None if scene_index_map is None else _np(scene_index_map, np.int32, (-1,))
        Tw, Ts = _np(measurement_in_world, np.float32, (16,)), _np(measurement_in_scene, np.float32, (16,))
        res = (C.c_int32 * 3)()
        rc = _lib.load().prs_map_merge(self._h, C.byref(params), _p(Tw), _p(Ts), _p(z), _p(d), z.shape[0], _p(c) if len(c) else None, len(c),
                                       None if im is None else _p(im), int(corr_from_aligner), res)
        _check(self._ctx, rc, "prs_map_merge")
        return int(res[0]), int(res[1]), int(res[2])

    def merge_closure(self, params, transform, measurement, measurement_desc, corr, scene_in_world=None, transform_is_scene_in_measurement=0,
                      corr_from_aligner=0, check=True):
        """the closure merger (closure_merger_params) on this map: measurement [n, 4] rows -> (n_merged, n_added, status).  The map's
        statistics arrays are kept up; no frame is counted.  check=False returns a pair's error code instead of raising"""
        z = _np(measurement, np.float32, (-1, 4))
        d = _np(measurement_desc, np.uint8, (-1, 32))
        c = np.ascontiguousarray(corr, dtype=CORR_DTYPE)
        T = _np(transform, np.float32, (16,))
        W = None if scene_in_world is None else _np(scene_in_world, np.float32, (16,))
        res = (C.c_int32 * 3)()
        rc = _lib.load().prs_map_merge_closure(self._h, C.byref(params), _p(T), int(transform_is_scene_in_measurement),
                                               None if W is None else _p(W), _p(z) if len(z) else None, _p(d) if len(z) else None,
                                               z.shape[0], _p(c) if len(c) else None, len(c), int(corr_from_aligner), res)
        if check or rc != int(res[2]):
            _check(self._ctx, rc, "prs_map_merge_closure")
        return int(res[0]), int(res[1]), int(res[2])

    def scene(self):
        """-> dict(coords [n,3], state [n,3], desc [n,32], n_opt [n], inlier [n])"""
        cap = self.capacity
        coords, state = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
        desc, n_opt, inl = np.zeros((cap, 32), np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
        n = C.c_int32(0)
        rc = _lib.load().prs_map_get_scene(self._h, cap, _p(coords), _p(state), _p(desc), _p(n_opt), _p(inl), C.byref(n))
        _check(self._ctx, rc, "prs_map_get_scene")
        k = n.value
        return dict(coords=coords[:k].copy(), state=state[:k].copy(), desc=desc[:k].copy(), n_opt=n_opt[:k].copy(), inlier=inl[:k].copy())


# ---- closure merger (the tracker slice's closure_merger: MergerCorrespondencePointIntensityDescriptor3f / ..ProjectiveDepth3D) ----
CLOSURE_XYZ, CLOSURE_UVD = _lib.CLOSURE_XYZ, _lib.CLOSURE_UVD
_CLOSURE_STATS = (("state", np.float32, 4), ("covariance", np.float32, 9), ("n_opt", np.uint32, 0), ("inlier", np.uint8, 0),
                  ("n_meas", np.uint32, 0))


def closure_merger_params(group, camera, measurement_kind="xyz", **overrides):
    """prs_closure_merger_params from a configs.py `closure_merger` group and `camera` (canvas + camera matrix); measurement_kind
    "xyz" (MergerCorrespondencePointIntensityDescriptor3f) or "uvd" (MergerCorrespondenceProjectiveDepth3D); overrides by field name"""
    p = _lib.ClosureMergerParams()
    p.measurement_kind = {"xyz": CLOSURE_XYZ, "uvd": CLOSURE_UVD}[measurement_kind]
    p.enable_binning = int(group["enable_binning"])
    p.number_of_row_bins, p.number_of_col_bins = int(group.get("number_of_row_bins", 10)), int(group.get("number_of_col_bins", 30))
    p.canvas_rows, p.canvas_cols = int(camera["rows"]), int(camera["cols"])
    p.fx, p.fy, p.cx, p.cy = camera["fx"], camera["fy"], camera["cx"], camera["cy"]
    p.maximum_distance_geometry_squared = group["maximum_distance_geometry_squared"]
    p.maximum_response = group["maximum_response"]
    p.target_number_of_merges = int(group["target_number_of_merges"])
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def closure_merge(ctx, params, scene, measurement, measurement_desc, corr, transform, scene_in_world=None,
                  transform_is_scene_in_measurement=0, corr_from_aligner=0, check=True):
    """host arrays, one pair.  scene: dict(coords [capacity, 4], desc [capacity, 32], n_points, and any of state [capacity, 4],
    covariance [capacity, 9], n_opt, inlier, n_meas [capacity]); measurement [n, 4] rows ((x, y, z, -) or (u, v, d, -)).
    -> (scene after: a new dict, (n_merged, n_added, status)).  check=False returns a pair's error code instead of raising"""
    out = dict(coords=_np(scene["coords"], np.float32, (-1, 4)).copy(), desc=_np(scene["desc"], np.uint8, (-1, 32)).copy())
    cap = out["coords"].shape[0]
    for name, dt, width in _CLOSURE_STATS:
        if scene.get(name) is not None:
            out[name] = _np(scene[name], dt, (cap, width) if width else (cap,)).copy()
    z = _np(measurement, np.float32, (-1, 4))
    d = _np(measurement_desc, np.uint8, (-1, 32))
    c = np.ascontiguousarray(corr, dtype=CORR_DTYPE)
    T = _np(transform, np.float32, (16,))
    W = None if scene_in_world is None else _np(scene_in_world, np.float32, (16,))
    n = C.c_int32(int(scene["n_points"]))
    res = (C.c_int32 * 3)()
    opt = lambda name: _p(out[name]) if name in out else None  # noqa: E731
    rc = _lib.load().prs_closure_merge(ctx._h, C.byref(params), cap, C.byref(n), _p(out["coords"]), _p(out["desc"]), opt("state"),
                                       opt("covariance"), opt("n_opt"), opt("inlier"), opt("n_meas"), None if W is None else _p(W),
                                       _p(z) if len(z) else None, _p(d) if len(z) else None, z.shape[0], _p(c) if len(c) else None, len(c),
                                       int(corr_from_aligner), _p(T), int(transform_is_scene_in_measurement), res)
    if check or rc != int(res[2]):
        _check(ctx, rc, "prs_closure_merge")
    out["n_points"] = n.value
    return out, (int(res[0]), int(res[1]), int(res[2]))


class ClosureMergeBatch:
    """B (scene, measurement cloud) pairs resident in HBM in the layout of prs_closure_merge_batch.  The tensors may be another
    batch's: from_closures points them at a LoopClosureBatch so that the merger follows the matcher and the aligner on one stream."""

    def __init__(self, device, batch, capacity, measurement_stride, corr_stride, with_stats=True, with_gate=False):
        import torch
        dev = torch.device("cuda", device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.batch, self.capacity = int(batch), int(capacity)
        self.measurement_stride, self.corr_stride = int(measurement_stride), int(corr_stride)
        self.coords, self.desc, self.n_points = z((batch, capacity, 4), torch.float32), z((batch, capacity, 32), torch.uint8), z((batch,), torch.int32)
        self.state = z((batch, capacity, 4), torch.float32) if with_stats else None
        self.covariance = z((batch, capacity, 9), torch.float32) if with_stats else None
        self.n_opt = z((batch, capacity), torch.int32) if with_stats else None
        self.inlier = z((batch, capacity), torch.uint8) if with_stats else None
        self.n_meas = z((batch, capacity), torch.int32) if with_stats else None
        self.scene_in_world = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(batch, 1).contiguous() if with_stats else None
        self.measurement = z((batch, measurement_stride, 4), torch.float32)
        self.measurement_desc = z((batch, measurement_stride, 32), torch.uint8)
        self.n_measured = z((batch,), torch.int32)
        self.corr, self.n_corr = z((batch, max(corr_stride, 1), 3), torch.int32), z((batch,), torch.int32)
        self.transform = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(batch, 1).contiguous()
        self.gate = z((batch, C.sizeof(_lib.PointAlignResult) // 4), torch.int32) if with_gate else None
        self.result = z((batch, 3), torch.int32)
        self.corr_from_aligner, self.transform_is_scene_in_measurement = 0, 0

    @classmethod
    def from_closures(cls, closures):
        """the merger's batch over the tensors of a LoopClosureBatch that has run (or is enqueued): nothing is copied.  The scene is
        the candidate map (the aligner's MOVING cloud and descriptors, capacity = moving_stride, count = pairs.n_moving, which
        grows), the measurement the query (its FIXED cloud); corr / n_corr are the matcher's (corr_from_aligner = 1); transform is
        the aligner's X, movingInFixed = scene-in-measurement, so the inverse flag is set; the gate is the aligner's verdict."""
        import torch
        self = cls.__new__(cls)
        pairs, clouds = closures.pairs, closures.clouds
        self.batch, self.capacity = pairs.batch, pairs.moving_stride
        self.measurement_stride, self.corr_stride = pairs.fixed_stride, pairs.corr_stride
        self.coords, self.desc, self.n_points = pairs.moving, clouds.moving_desc, pairs.n_moving
        self.state = self.covariance = self.n_opt = self.inlier = self.n_meas = self.scene_in_world = None
        self.measurement, self.measurement_desc, self.n_measured = pairs.fixed, clouds.fixed_desc, pairs.n_fixed
        self.corr, self.n_corr = pairs.corr, pairs.n_corr
        self.transform, self.gate = pairs.X, pairs.result
        self.result = torch.zeros((pairs.batch, 3), dtype=torch.int32, device=pairs.moving.device)
        self.corr_from_aligner, self.transform_is_scene_in_measurement = 1, 1
        return self

    def upload(self, b, scene, measurement, measurement_desc, corr, transform, scene_in_world=None, accepted=None, n_measured=None,
               n_corr=None):
        """scene: the dict closure_merge takes (arrays of `capacity` rows).  n_measured / n_corr override the counts (tests of the
        count checks); accepted sets the gate's verdict for the pair"""
        import torch
        dev = self.coords.device
        put = lambda t, a: t.__setitem__(b, torch.from_numpy(np.ascontiguousarray(a)).to(dev))  # noqa: E731
        put(self.coords, _np(scene["coords"], np.float32, (self.capacity, 4)))
        put(self.desc, _np(scene["desc"], np.uint8, (self.capacity, 32)))
        self.n_points[b] = int(scene["n_points"])
        for name, dt, width in _CLOSURE_STATS:
            t = getattr(self, name)
            if t is not None and scene.get(name) is not None:
                a = _np(scene[name], dt, (self.capacity, width) if width else (self.capacity,))
                put(t, a.view(np.int32) if dt == np.uint32 else a)
        z, d = _np(measurement, np.float32, (-1, 4)), _np(measurement_desc, np.uint8, (-1, 32))
        if len(z):
            self.measurement[b, : len(z)] = torch.from_numpy(z).to(dev)
            self.measurement_desc[b, : len(z)] = torch.from_numpy(d).to(dev)
        self.n_measured[b] = len(z) if n_measured is None else int(n_measured)
        c = np.ascontiguousarray(corr, dtype=CORR_DTYPE)
        if len(c):
            self.corr[b, : len(c)] = torch.from_numpy(c.view(np.int32).reshape(-1, 3).copy()).to(dev)
        self.n_corr[b] = len(c) if n_corr is None else int(n_corr)
        put(self.transform, _np(transform, np.float32, (16,)))
        if self.scene_in_world is not None:
            put(self.scene_in_world, _np(np.eye(4) if scene_in_world is None else scene_in_world, np.float32, (16,)))
        if self.gate is not None:
            self.gate[b, _lib.PointAlignResult.accepted.offset // 4] = 1 if accepted is None else int(accepted)

    def descriptor(self):
        d = _lib.ClosureMergeBatch()
        d.batch, d.capacity, d.measurement_stride, d.corr_stride = self.batch, self.capacity, self.measurement_stride, self.corr_stride
        for name in ("coords", "desc", "n_points", "state", "covariance", "n_opt", "inlier", "n_meas", "scene_in_world", "measurement",
                     "measurement_desc", "n_measured", "corr", "n_corr", "transform", "gate", "result"):
            t = getattr(self, name)
            setattr(d, name, t.data_ptr() if t is not None else None)
        d.corr_from_aligner, d.transform_is_scene_in_measurement = int(self.corr_from_aligner), int(self.transform_is_scene_in_measurement)
        return d

    def result_of(self, b):
        """-> (n_merged, n_added, status)"""
        return tuple(int(v) for v in self.result[b].cpu().numpy())

    def scene_of(self, b):
        """the scene of pair b in the dict layout of closure_merge (whole capacity)"""
        out = dict(coords=self.coords[b].cpu().numpy().copy(), desc=self.desc[b].cpu().numpy().copy(), n_points=int(self.n_points[b].item()))
        for name, dt, _ in _CLOSURE_STATS:
            t = getattr(self, name)
            if t is not None:
                out[name] = t[b].cpu().numpy().view(dt).copy()
        return out


def closure_merge_batch(ctx, params, pairs):
    """enqueue the closure merger for every pair of the batch on the context stream (asynchronous, one launch)"""
    d = pairs.descriptor()
    return _run(ctx, "prs_closure_merge_batch_run", C.byref(params), C.byref(d))


def pose_compose_batch(ctx, prediction, X, pose_out):
    """pose_out[b] = prediction[b] * X[b]^-1 on device tensors of shape [B, 16] / [B, 4, 4] (asynchronous)"""
    batch = int(prediction.shape[0])
    return _run(ctx, "prs_pose_compose_batch", batch, prediction.data_ptr(), X.data_ptr(), pose_out.data_ptr())


def motion_predict_batch(ctx, pose_prev2, pose_prev1, pose_pred):
    """MotionModelConstantVelocity3D on the device: pose_pred = pose_prev1 * (pose_prev2^-1 * pose_prev1), [B, 4, 4] float32"""
    batch = int(pose_prev1.shape[0])
    return _run(ctx, "prs_motion_predict_batch", batch, pose_prev2.data_ptr(), pose_prev1.data_ptr(), pose_pred.data_ptr())


# ---- local-map manager: per-sequence splits, graph growth, trajectories (include/proslam_hip.h prs_session_*) ----
SESSION_NO_SPLIT, SESSION_SPLIT_VIEWPOINT, SESSION_SPLIT_LOST = _lib.SESSION_NO_SPLIT, _lib.SESSION_SPLIT_VIEWPOINT, _lib.SESSION_SPLIT_LOST


def session_params(cfg_split, split_information=1.0, lost_information=0.1, **overrides):
    """prs_session_params from a configs.py `split` group; the two informations are the arguments of the reference's makeNewMap
    calls (apps/app_benchmark.cpp:143, :167); overrides by field name"""
    p = _lib.SessionParams()
    p.local_map_distance = cfg_split["local_map_distance"]
    p.local_map_angle_distance_radians = cfg_split["local_map_angle_distance_radians"]
    p.split_information, p.lost_information = split_information, lost_information
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


class SessionBatch:
    """B tracking sessions resident in HBM: pose, previous pose and prediction in the current local map, the pose-table slot, the
    current node, the trajectory log and the per-frame status / reason.  step() is the one launch between align_batch and
    merge_batch: it reads `frames` (an AlignFrames: X, result, n_corr), writes the merger's per-frame inputs of `maps` (a MapBatch:
    frame, measurement_in_world, measurement_in_scene and maps.n_corr, which is pointed at this object's n_corr_merge), resets a
    finished map and grows `graphs` (a PoseGraphBatch with omega).  handover: a PlaceQueries (a LoopDetectorBatch's .queries) that
    receives every finished map as a query, or None; graph_id_base: optional int64 [B] device tensor added to the node index."""

    def __init__(self, device, maps, frames, graphs, frame_stride, handover=None, graph_id_base=None):
        import torch
        dev = torch.device("cuda", device)
        B = int(maps.batch)
        if int(frames.batch) != B or int(graphs.batch) != B or (handover is not None and int(handover.batch) != B):
            raise ValueError("maps, frames, graphs and the hand-over must hold the same number of sequences")
        self.batch, self.frame_stride = B, int(frame_stride)
        self.maps, self.frames, self.graphs, self.handover, self.graph_id_base = maps, frames, graphs, handover, graph_id_base
        eye = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
        self.pose, self.prev, self.prediction = eye.clone(), eye.clone(), eye.clone()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.slot, self.cur_node, self.n_frames = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.frame_node = z((B, self.frame_stride), torch.int32)
        self.frame_pose = z((B, self.frame_stride, 16), torch.float32)
        self.status, self.reason = z((B,), torch.int32), z((B,), torch.int32)
        self.n_corr_merge = z((B,), torch.int32)
        self.trajectory = z((B, self.frame_stride, 16), torch.float32)
        maps.n_corr = self.n_corr_merge
        self.reset()

    def reset(self):
        """frame 0 comes next: identity poses, empty log, and every graph holds node 0 alone (X = I, fixed)"""
        import torch
        g = self.graphs
        eye = torch.eye(4, dtype=torch.float32, device=self.pose.device).reshape(1, 16)
        for t in (self.pose, self.prev, self.prediction):
            t.copy_(eye.expand(self.batch, 16))
        for t in (self.slot, self.cur_node, self.n_frames, self.status, self.reason, self.n_corr_merge):
            t.zero_()
        g.X[:, 0] = torch.eye(4, dtype=torch.float64, device=g.X.device).reshape(16)
        g.fixed[:, 0] = 1
        g.n_nodes.fill_(1)
        g.n_edges.zero_()

    def descriptor(self):
        m, f, g, h = self.maps, self.frames, self.graphs, self.handover
        d = _lib.SessionBatch()
        d.batch, d.frame_stride, d.capacity = self.batch, self.frame_stride, m.capacity
        d.node_stride, d.edge_stride = g.node_stride, g.edge_stride
        for name in ("pose", "prev", "prediction", "slot", "cur_node", "n_frames", "frame_node", "frame_pose", "status", "reason",
                     "n_corr_merge"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.X, d.result, d.n_corr = f.X.data_ptr(), f.result.data_ptr(), f.n_corr.data_ptr()
        d.coords, d.desc, d.n_points, d.n_meas = m.coords.data_ptr(), m.desc.data_ptr(), m.n_points.data_ptr(), m.n_meas.data_ptr()
        d.frame = m.frame.data_ptr()
        d.measurement_in_world, d.measurement_in_scene = m.measurement_in_world.data_ptr(), m.measurement_in_scene.data_ptr()
        d.graph_X, d.fixed, d.n_nodes = g.X.data_ptr(), g.fixed.data_ptr(), g.n_nodes.data_ptr()
        d.from_, d.to, d.Z, d.n_edges = g.src.data_ptr(), g.dst.data_ptr(), g.Z.data_ptr(), g.n_edges.data_ptr()
        d.omega = g.omega.data_ptr() if g.omega is not None else None
        if h is not None:
            d.handover_stride = h.query_stride
            d.handover_desc, d.handover_xyz = h.desc.data_ptr(), h.xyz.data_ptr()
            d.handover_n_query, d.handover_graph_id = h.n_query.data_ptr(), h.graph_id.data_ptr()
        d.graph_id_base = self.graph_id_base.data_ptr() if self.graph_id_base is not None else None
        return d

    def step(self, ctx, params):
        """enqueue the per-frame step of every sequence (asynchronous, one launch); per-sequence status lands in self.status"""
        d = self.descriptor()
        return _run(ctx, "prs_session_step_batch", C.byref(params), C.byref(d))

    def unroll(self, ctx):
        """enqueue the unrolling of the logged trajectories through the graphs as they stand -> self.trajectory [B, frame_stride, 16]
        (rows from n_frames[b] on are left as they were)"""
        d = self.descriptor()
        rc = _lib.load().prs_session_unroll_batch(ctx._h, C.byref(d), self.trajectory.data_ptr())
        _check(ctx, rc, "prs_session_unroll_batch")
        return self.trajectory

    def result_of(self, b):
        """dict(status, reason, n_frames, slot, cur_node, pose, prev, prediction [4, 4], frame_node [n], frame_pose [n, 4, 4])"""
        n = min(max(int(self.n_frames[b].item()), 0), self.frame_stride)
        m44 = lambda t: t[b].cpu().numpy().reshape(4, 4).copy()  # noqa: E731
        return dict(status=int(self.status[b].item()), reason=int(self.reason[b].item()), n_frames=int(self.n_frames[b].item()),
                    slot=int(self.slot[b].item()), cur_node=int(self.cur_node[b].item()), pose=m44(self.pose), prev=m44(self.prev),
                    prediction=m44(self.prediction), frame_node=self.frame_node[b, :n].cpu().numpy().copy(),
                    frame_pose=self.frame_pose[b, :n].cpu().numpy().reshape(-1, 4, 4).copy())


# ---- trajectory evaluator: ATE, RPE and the KITTI metric on the device (include/proslam_hip.h prs_trajectory_*) ----
TRAJ_ALIGN = {"none": _lib.TRAJ_ALIGN_NONE, "first": _lib.TRAJ_ALIGN_FIRST, "rigid": _lib.TRAJ_ALIGN_RIGID}
KITTI_LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)  # the devkit's
_TRAJ_NP = {C.c_int32: np.int32, C.c_double: np.float64}
_TRAJ_RESULT_DTYPE = np.dtype([(name, _TRAJ_NP[ct._type_], (ct._length_,)) if hasattr(ct, "_length_") else (name, _TRAJ_NP[ct])
                               for name, ct in _lib.TrajectoryResult._fields_])
assert _TRAJ_RESULT_DTYPE.itemsize == C.sizeof(_lib.TrajectoryResult)


def trajectory_params(align="rigid", rpe_delta=1, kitti_step=10, lengths=KITTI_LENGTHS):
    """prs_trajectory_params: align "none" / "first" / "rigid" (or a PRS_TRAJ_ALIGN_* value), the frames between the two ends of a
    relative pose, and the KITTI block's start step (0 skips it) and lengths in metres (the defaults are the devkit's)"""
    p = _lib.TrajectoryParams()
    p.align = TRAJ_ALIGN[align] if isinstance(align, str) else int(align)
    p.rpe_delta, p.kitti_step = int(rpe_delta), int(kitti_step)
    if len(lengths) > 8:
        raise ValueError("at most 8 lengths")
    p.n_lengths = len(lengths)
    for i, v in enumerate(lengths):
        p.lengths[i] = v
    return p


def _rows16(poses):
    """[n, 4, 4], [n, 16] or [n, 12] (KITTI rows) -> float32 [n, 16]"""
    a = np.asarray(poses, np.float32)
    a = a.reshape(a.shape[0], -1) if a.ndim == 3 else a
    if a.shape[1] == 12:
        a = np.concatenate([a, np.tile(np.array([[0, 0, 0, 1]], np.float32), (a.shape[0], 1))], axis=1)
    if a.ndim != 2 or a.shape[1] != 16:
        raise ValueError("poses must be [n, 4, 4], [n, 16] or [n, 12]")
    return np.ascontiguousarray(a)


def _traj_result_dict(rec):
    d = {name: (rec[name].copy() if rec[name].ndim else rec[name].item()) for name in _TRAJ_RESULT_DTYPE.names}
    d["S"] = d["S"].reshape(4, 4)
    return d


class TrajectoryEvalBatch:
    """B trajectories and their ground truth resident in HBM, in the layout prs_session_unroll_batch writes ([B, frame_stride, 16]).
    Owns ground_truth, valid, result, frame_error and workspace; estimate and n_frames are its own too unless from_session() bound
    a SessionBatch's trajectory and n_frames in place.  with_valid=False passes no valid array: every row k < n_frames[b] counts."""

    def __init__(self, device, batch, frame_stride, with_valid=True, estimate=None, n_frames=None):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.frame_stride = int(batch), int(frame_stride)
        B, F = self.batch, self.frame_stride
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.estimate = estimate if estimate is not None else z((B, F, 16), torch.float32)
        self.n_frames = n_frames if n_frames is not None else z((B,), torch.int32)
        self.ground_truth = z((B, F, 16), torch.float32)
        self.valid = torch.ones((B, F), dtype=torch.uint8, device=dev) if with_valid else None
        self.result = z((B, C.sizeof(_lib.TrajectoryResult)), torch.uint8)
        self.frame_error = z((B, F), torch.float32)
        self.workspace = z((B, F), torch.float64)

    @classmethod
    def from_session(cls, sess, with_valid=True):
        """evaluates sess.trajectory (what SessionBatch.unroll writes) over sess.n_frames rows, in place: no copy"""
        return cls(sess.trajectory.device.index, sess.batch, sess.frame_stride, with_valid=with_valid, estimate=sess.trajectory,
                   n_frames=sess.n_frames)

    def set_ground_truth(self, b, poses, valid=None):
        """uploads sequence b's ground truth, row k for estimate row k; rows from len(poses) on count as having none.  valid: optional
        [len(poses)] mask, e.g. formats.associate's"""
        import torch
        rows = _rows16(poses)
        n = rows.shape[0]
        if n > self.frame_stride:
            raise ValueError("more ground-truth rows than frame_stride")
        self.ground_truth[b, :n] = torch.from_numpy(rows).to(self.ground_truth.device)
        if self.valid is not None:
            self.valid[b] = 0
            v = np.ones(n, np.uint8) if valid is None else (np.asarray(valid).reshape(n) != 0).astype(np.uint8)
            self.valid[b, :n] = torch.from_numpy(v).to(self.valid.device)
        elif valid is not None:
            raise ValueError("this batch was made with_valid=False")

    def set_estimate(self, b, poses):
        """uploads sequence b's estimate and sets n_frames[b] (for trajectories that do not come from a session)"""
        import torch
        rows = _rows16(poses)
        n = rows.shape[0]
        if n > self.frame_stride:
            raise ValueError("more rows than frame_stride")
        self.estimate[b, :n] = torch.from_numpy(rows).to(self.estimate.device)
        self.n_frames[b] = n

    def descriptor(self):
        d = _lib.TrajectoryBatch()
        d.batch, d.frame_stride = self.batch, self.frame_stride
        d.estimate, d.ground_truth, d.n_frames = self.estimate.data_ptr(), self.ground_truth.data_ptr(), self.n_frames.data_ptr()
        d.valid = self.valid.data_ptr() if self.valid is not None else None
        d.result, d.frame_error, d.workspace = self.result.data_ptr(), self.frame_error.data_ptr(), self.workspace.data_ptr()
        return d

    def evaluate(self, ctx, params):
        """enqueue the evaluation of every sequence (asynchronous, one launch); per-sequence status lands in the results"""
        d = self.descriptor()
        return _run(ctx, "prs_trajectory_eval_batch", C.byref(params), C.byref(d))

    def results(self):
        """the B results as dicts (field names of prs_trajectory_result, S as [4, 4]); copies `result` to the host when called"""
        rec = np.frombuffer(self.result.cpu().numpy().tobytes(), dtype=_TRAJ_RESULT_DTYPE)
        return [_traj_result_dict(rec[b]) for b in range(self.batch)]


def trajectory_eval(ctx, params, estimate, ground_truth, valid=None):
    """one sequence from host arrays ([n, 4, 4], [n, 16] or [n, 12] each, row k of one for row k of the other) -> the result dict plus
    "frame_error" (float32 [n], -1 where the row is not valid)"""
    est, gt = _rows16(estimate), _rows16(ground_truth)
    if est.shape != gt.shape:
        raise ValueError("estimate and ground truth must have the same number of rows")
    n = est.shape[0]
    ev = TrajectoryEvalBatch(ctx.device, 1, max(n, 1), with_valid=valid is not None)
    ev.set_estimate(0, est)
    ev.set_ground_truth(0, gt, valid)
    ev.evaluate(ctx, params)
    out = ev.results()[0]
    out["frame_error"] = ev.frame_error[0, :n].cpu().numpy().copy()
    return out


# ---- map re-entry: archive finished maps, reload one on a closure (include/proslam_hip.h prs_map_archive, prs_session_reenter_batch) ----
def reentry_params(group, **overrides):
    """prs_reentry_params from a configs.REENTRY group (MultiRelocalizer3D's own values); overrides by field name"""
    p = _lib.ReentryParams()
    p.max_translation = group["max_translation"]
    p.relocalize_min_inliers = group["relocalize_min_inliers"]
    p.relocalize_min_inliers_ratio = group["relocalize_min_inliers_ratio"]
    p.relocalize_max_chi_inliers = group["relocalize_max_chi_inliers"]
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


class MapArchive:
    """prs_map_archive: slot_stride slots per sequence, each the per-landmark arrays of a MapBatch (and, with_history, its measurement
    history and pose table), plus slot_of_node [B, node_stride] (-1 = none), n_slots and status.  The tensors own the memory."""

    ROW_ARRAYS = ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas")

    def __init__(self, device, maps, node_stride, slot_stride, with_history=False):
        import torch
        dev = torch.device("cuda", device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        B, S, cap = int(maps.batch), int(slot_stride), int(maps.capacity)
        self.batch, self.capacity, self.slot_stride, self.node_stride = B, cap, S, int(node_stride)
        self.with_history = bool(with_history)
        if self.with_history and maps.max_measurements < 1:
            raise ValueError("the maps keep no measurement history to archive")
        self.max_measurements, self.max_frames = (maps.max_measurements, maps.max_frames) if self.with_history else (0, 0)
        self.coords, self.desc = z((B, S, cap, 4), torch.float32), z((B, S, cap, 32), torch.uint8)
        self.state, self.covariance = z((B, S, cap, 4), torch.float32), z((B, S, cap, 9), torch.float32)
        self.n_opt, self.inlier, self.n_meas = z((B, S, cap), torch.int32), z((B, S, cap), torch.uint8), z((B, S, cap), torch.int32)
        self.n_points, self.next_frame = z((B, S), torch.int32), z((B, S), torch.int32)
        self.meas = z((B, S, cap, self.max_measurements, MapBatch.MEAS_WORDS), torch.int32) if self.with_history else None
        self.poses = z((B, S, self.max_frames, MapBatch.POSE_WORDS), torch.float32) if self.with_history else None
        self.slot_of_node = torch.full((B, self.node_stride), -1, dtype=torch.int32, device=dev)
        self.n_slots, self.status = z((B,), torch.int32), z((B,), torch.int32)

    def clear(self):
        self.slot_of_node.fill_(-1)
        self.n_slots.zero_()
        self.status.zero_()

    def descriptor(self):
        d = _lib.MapArchive()
        d.batch, d.capacity, d.slot_stride, d.node_stride = self.batch, self.capacity, self.slot_stride, self.node_stride
        d.max_measurements, d.max_frames = self.max_measurements, self.max_frames
        for name in self.ROW_ARRAYS + ("n_points", "next_frame", "slot_of_node", "n_slots", "status"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.meas = self.meas.data_ptr() if self.meas is not None else None
        d.poses = self.poses.data_ptr() if self.poses is not None else None
        return d

    def slot_of(self, b, node):
        """the archived map of `node` in the layout of ClosureMergeBatch.scene_of (whole capacity) + next_frame, or None"""
        s = int(self.slot_of_node[b, node].item())
        if s < 0:
            return None
        out = dict(slot=s, n_points=int(self.n_points[b, s].item()), next_frame=int(self.next_frame[b, s].item()))
        for name in self.ROW_ARRAYS:
            out[name] = getattr(self, name)[b, s].cpu().numpy().copy()
        return out


class ReentryBatch:
    """map re-entry for the B sequences of a SessionBatch: step() is the session step that also archives a finished map
    (prs_session_step_archive_batch, in the place of session.step()), reenter() the launch that follows the detector, append_closures
    and the optimiser (prs_session_reenter_batch), merge_view a ClosureMergeBatch over the live MapBatch and reenter()'s outputs --
    nothing copied -- for closure_merge_batch; merge_batch(maps) runs last.  bank_detector: a BankDetectorBatch whose .queries is the
    session's hand-over."""

    def __init__(self, session, maps, bank_detector, archive):
        import torch
        det = bank_detector
        if session.handover is not det.queries:
            raise ValueError("the session must hand its finished maps over to the detector's queries")
        if int(archive.batch) != session.batch or int(det.batch) != session.batch or maps is not session.maps:
            raise ValueError("session, maps, detector and archive must hold the same sequences")
        self.session, self.maps, self.detector, self.archive = session, maps, det, archive
        dev = session.pose.device
        B, pairs = session.batch, det.closures.pairs
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.batch, self.corr_stride = B, int(pairs.corr_stride)
        self.reentered, self.status = z((B,), torch.int32), z((B,), torch.int32)
        self.merge_corr, self.merge_n_corr = z((B, self.corr_stride, 3), torch.int32), z((B,), torch.int32)
        self.merge_transform = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
        self.scene_in_world = self.merge_transform.clone()
        self.gate = z((B, C.sizeof(_lib.PointAlignResult) // 4), torch.int32)
        # the closure merger's batch: the live map as the scene, the hand-over slot (the finished map) as the XYZ measurement cloud
        v = ClosureMergeBatch.__new__(ClosureMergeBatch)
        q = det.queries
        v.batch, v.capacity, v.measurement_stride, v.corr_stride = B, maps.capacity, int(q.query_stride), self.corr_stride
        v.coords, v.desc, v.n_points = maps.coords, maps.desc, maps.n_points
        v.state, v.covariance, v.n_opt, v.inlier, v.n_meas = maps.state, maps.covariance, maps.n_opt, maps.inlier, maps.n_meas
        v.scene_in_world = self.scene_in_world
        v.measurement, v.measurement_desc, v.n_measured = q.xyz, q.desc, q.n_query
        v.corr, v.n_corr, v.transform, v.gate = self.merge_corr, self.merge_n_corr, self.merge_transform, self.gate
        v.result = z((B, 3), torch.int32)
        v.corr_from_aligner, v.transform_is_scene_in_measurement = 1, 1
        self.merge_view = v

    def descriptor(self):
        det, pairs = self.detector, self.detector.closures.pairs
        d = _lib.ReentryBatch()
        d.max_candidates, d.map_stride, d.corr_stride = det.max_candidates, det.bank.map_stride, self.corr_stride
        d.candidates_flat, d.node_of_map = det.links.candidates_flat.data_ptr(), det.bank.node_of_map.data_ptr()
        d.result, d.X, d.corr, d.n_corr = pairs.result.data_ptr(), pairs.X.data_ptr(), pairs.corr.data_ptr(), pairs.n_corr.data_ptr()
        d.n_measured = self.maps.n_measured.data_ptr()
        for name in ("reentered", "status", "merge_corr", "merge_n_corr", "merge_transform", "scene_in_world", "gate"):
            setattr(d, name, getattr(self, name).data_ptr())
        return d

    def step(self, ctx, params):
        """enqueue the per-frame step of every sequence with the archive behind it (asynchronous, one launch); the session's status
        lands in session.status, the archive's in archive.status"""
        s, m, a = self.session.descriptor(), self.maps.descriptor(), self.archive.descriptor()
        return _run(ctx, "prs_session_step_archive_batch", C.byref(params), C.byref(s), C.byref(m), C.byref(a))

    def reenter(self, ctx, params):
        """enqueue the re-entry of every sequence whose split found an accepted closure into an archived map (asynchronous, one
        launch); per-sequence status lands in self.status, the decision in self.reentered"""
        s, m, a, r = self.session.descriptor(), self.maps.descriptor(), self.archive.descriptor(), self.descriptor()
        return _run(ctx, "prs_session_reenter_batch", C.byref(params), C.byref(s), C.byref(m), C.byref(a), C.byref(r))

    def result_of(self, b):
        """dict(status, reentered, cur_node, n_corr, transform [4, 4], scene_in_world [4, 4], gate (the winner's aligner result))"""
        m44 = lambda t: t[b].cpu().numpy().reshape(4, 4).copy()  # noqa: E731
        gate = _result_dict(_lib.PointAlignResult.from_buffer_copy(self.gate[b].cpu().numpy().tobytes()))
        return dict(status=int(self.status[b].item()), reentered=int(self.reentered[b].item()),
                    cur_node=int(self.session.cur_node[b].item()), n_corr=int(self.merge_n_corr[b].item()),
                    transform=m44(self.merge_transform), scene_in_world=m44(self.scene_in_world), gate=gate)


# ---- world map: one landmark cloud per sequence from archive, live map and graph (include/proslam_hip.h prs_world_map_*) ----
def world_map_params(min_n_opt=0, require_inlier=False, include_live=True, refresh_state=False):
    """prs_world_map_params: keep landmarks optimised at least min_n_opt times (and, require_inlier, flagged inliers); include_live
    takes the current node's map from the live arrays; refresh_state rewrites `state` of every chosen map from the graph"""
    p = _lib.WorldMapParams()
    if int(min_n_opt) < 0:
        raise ValueError("min_n_opt must not be negative")
    p.min_n_opt = int(min_n_opt)
    p.require_inlier, p.include_live, p.refresh_state = int(bool(require_inlier)), int(bool(include_live)), int(bool(refresh_state))
    return p


class WorldMapBatch:
    """the world cloud of the B sequences of a SessionBatch: the maps of `archive` (a MapArchive) and the live `maps` (the session's
    MapBatch) carried into the world frame by the session's graphs as they stand.  Owns the output tensors (out_stride rows per
    sequence) and the workspace.  outputs: which of the optional arrays ("desc", "node", "row", "n_opt", "bounds") are kept."""

    OPTIONAL = ("desc", "node", "row", "n_opt", "bounds")

    def __init__(self, session, maps, archive, out_stride, outputs=OPTIONAL):
        import torch
        if maps is not session.maps or int(archive.batch) != session.batch:
            raise ValueError("session, maps and archive must hold the same sequences")
        if set(outputs) - set(self.OPTIONAL):
            raise ValueError("outputs: a subset of %s" % (self.OPTIONAL,))
        self.session, self.maps, self.archive = session, maps, archive
        dev = session.pose.device
        B, n = session.batch, int(out_stride)
        if n < 1:
            raise ValueError("out_stride must be at least 1")
        self.batch, self.out_stride = B, n
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.xyz = z((B, n, 4), torch.float32)
        self.desc = z((B, n, 32), torch.uint8) if "desc" in outputs else None
        self.node = z((B, n), torch.int32) if "node" in outputs else None
        self.row = z((B, n), torch.int32) if "row" in outputs else None
        self.n_opt = z((B, n), torch.int32) if "n_opt" in outputs else None
        self.bounds = z((B, 6), torch.float32) if "bounds" in outputs else None
        self.n_out, self.n_total, self.n_nonfinite = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.status = z((B,), torch.int32)
        nbytes = int(_lib.load().prs_world_map_workspace_bytes(B, archive.slot_stride, maps.capacity))
        if nbytes < 1:
            raise ValueError("batch, slot_stride and capacity must be at least 1")
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, count_only=False):
        d = _lib.WorldMapBatch()
        d.out_stride = self.out_stride
        for name in ("n_out", "n_total", "n_nonfinite", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        if not count_only:
            for name in ("xyz",) + self.OPTIONAL:
                t = getattr(self, name)
                setattr(d, name, t.data_ptr() if t is not None else None)
        return d

    def _launch(self, ctx, params, count_only):
        s, m, a, d = self.session.descriptor(), self.maps.descriptor(), self.archive.descriptor(), self.descriptor(count_only)
        return _run(ctx, "prs_world_map_batch_run", C.byref(params), C.byref(s), C.byref(m), C.byref(a), C.byref(d))

    def run(self, ctx, params):
        """enqueue the export of every sequence's cloud (asynchronous); per-sequence status lands in self.status"""
        return self._launch(ctx, params, False)

    def count(self, ctx, params):
        """enqueue the count-only call (asynchronous): n_total, n_nonfinite and status, n_out = 0; sizes an output"""
        return self._launch(ctx, params, True)

    def cloud_of(self, b):
        """dict of numpy arrays trimmed to n_out rows (xyz [n, 4] and the optional arrays that are kept) plus n_out, n_total,
        n_nonfinite, bounds [6] and status; copies to the host when called"""
        n = min(max(int(self.n_out[b].item()), 0), self.out_stride)
        out = dict(n_out=n, n_total=int(self.n_total[b].item()), n_nonfinite=int(self.n_nonfinite[b].item()),
                   status=int(self.status[b].item()), xyz=self.xyz[b, :n].cpu().numpy().copy())
        for name in ("desc", "node", "row", "n_opt"):
            t = getattr(self, name)
            if t is not None:
                out[name] = t[b, :n].cpu().numpy().copy()
        out["bounds"] = self.bounds[b].cpu().numpy().copy() if self.bounds is not None else None
        return out


# ---- world voxel filter: one row per voxel of a world cloud (include/proslam_hip.h prs_world_voxel_*) ----
VOXEL_REPRESENTATIVE, VOXEL_MEAN = 0, 1
_VOXEL_POSITIONS = {"representative": VOXEL_REPRESENTATIVE, "mean": VOXEL_MEAN}


def world_voxel_params(voxel_size, position="representative"):
    """prs_world_voxel_params: the voxel's edge in metres (finite, > 0, also as a float32) and where the fused row lies:
    "representative" (the best-optimised row's own coordinates) or "mean" (the voxel's rows averaged)"""
    p = _lib.WorldVoxelParams()
    p.voxel_size = float(voxel_size)
    if not (np.isfinite(p.voxel_size) and p.voxel_size > 0.0):
        raise ValueError("voxel_size must be finite and positive as a float32")
    if position not in _VOXEL_POSITIONS:
        raise ValueError("position: one of %s" % (sorted(_VOXEL_POSITIONS),))
    p.position = _VOXEL_POSITIONS[position]
    return p


class WorldVoxelBatch:
    """the voxel-grid filter of B clouds of in_stride rows: owns the output tensors (out_stride rows per sequence), the hash tables
    (table_stride slots per sequence, a power of two; default: the next one >= 2 * in_stride) and the workspace.  outputs: which of the
    optional arrays ("index", "count", "desc", "node", "row", "n_opt") are kept.  A cloud is an ops.WorldMapBatch, whose tensors are
    read in place, or a dict of device tensors: xyz [B, in_stride, 4] float32 and n_out [B] int32, optionally n_opt, desc, node, row."""

    OPTIONAL = ("index", "count", "desc", "node", "row", "n_opt")
    INPUTS = ("n_opt", "desc", "node", "row")

    def __init__(self, batch, in_stride, out_stride, table_stride=None, outputs=OPTIONAL, device=0):
        import torch
        if set(outputs) - set(self.OPTIONAL):
            raise ValueError("outputs: a subset of %s" % (self.OPTIONAL,))
        B, N, n = int(batch), int(in_stride), int(out_stride)
        if B < 1 or N < 1 or n < 1:
            raise ValueError("batch, in_stride and out_stride must be at least 1")
        T = 1 << (2 * N - 1).bit_length() if table_stride is None else int(table_stride)
        if T < 1 or T & (T - 1):
            raise ValueError("table_stride must be a power of two")
        self.batch, self.in_stride, self.out_stride, self.table_stride = B, N, n, T
        dev = torch.device("cuda", device) if isinstance(device, int) else device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.xyz = z((B, n, 4), torch.float32)
        self.index = z((B, n), torch.int32) if "index" in outputs else None
        self.voxel_count = z((B, n), torch.int32) if "count" in outputs else None  # "count": count() is the count-only call
        self.desc = z((B, n, 32), torch.uint8) if "desc" in outputs else None
        self.node = z((B, n), torch.int32) if "node" in outputs else None
        self.row = z((B, n), torch.int32) if "row" in outputs else None
        self.n_opt = z((B, n), torch.int32) if "n_opt" in outputs else None
        self.n_out, self.n_voxels, self.status = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.n_nonfinite, self.n_outside = z((B,), torch.int32), z((B,), torch.int32)
        self.workspace = z((int(_lib.load().prs_world_voxel_workspace_bytes(B, N, T)),), torch.uint8)

    def descriptor(self, cloud, count_only=False):
        get = (lambda k: cloud.get(k)) if isinstance(cloud, dict) else (lambda k: getattr(cloud, k))  # noqa: E731
        xyz, n = get("xyz"), get("n_out")
        if tuple(xyz.shape) != (self.batch, self.in_stride, 4) or tuple(n.shape) != (self.batch,):
            raise ValueError("the cloud holds xyz %s and n_out %s, this filter was sized for [%d, %d, 4] and [%d]"
                             % (tuple(xyz.shape), tuple(n.shape), self.batch, self.in_stride, self.batch))
        d = _lib.WorldVoxelBatch()
        d.batch, d.in_stride, d.out_stride, d.table_stride = self.batch, self.in_stride, self.out_stride, self.table_stride
        d.in_xyz, d.in_n = xyz.data_ptr(), n.data_ptr()
        for name in self.INPUTS:
            t = get(name)
            setattr(d, "in_" + name, t.data_ptr() if t is not None else None)
        for name in ("n_out", "n_voxels", "n_nonfinite", "n_outside", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        if not count_only:
            for name in ("xyz",) + self.OPTIONAL:
                t = self.tensor(name)
                setattr(d, name, t.data_ptr() if t is not None else None)
        return d

    def tensor(self, name):
        """the output tensor of that name ("xyz", one of OPTIONAL or a per-sequence count), None when it is not kept"""
        return getattr(self, "voxel_count" if name == "count" else name)

    def _launch(self, ctx, params, cloud, count_only):
        d = self.descriptor(cloud, count_only)
        return _run(ctx, "prs_world_voxel_batch_run", C.byref(params), C.byref(d))

    def run(self, ctx, params, cloud):
        """enqueue the filter of every sequence's cloud (asynchronous); per-sequence status lands in self.status"""
        return self._launch(ctx, params, cloud, False)

    def count(self, ctx, params, cloud):
        """enqueue the count-only call (asynchronous): n_voxels, n_nonfinite, n_outside and status, n_out = 0; sizes an output"""
        return self._launch(ctx, params, cloud, True)

    def cloud_of(self, b):
        """dict of numpy arrays trimmed to n_out rows, in the shape of WorldMapBatch.cloud_of (n_total is the number of voxels, bounds
        None) plus index, count, n_voxels and n_outside; copies to the host when called"""
        n = min(max(int(self.n_out[b].item()), 0), self.out_stride)
        nv = int(self.n_voxels[b].item())
        out = dict(n_out=n, n_total=nv, n_voxels=nv, n_nonfinite=int(self.n_nonfinite[b].item()), n_outside=int(self.n_outside[b].item()),
                   status=int(self.status[b].item()), xyz=self.xyz[b, :n].cpu().numpy().copy(), bounds=None)
        for name in self.OPTIONAL:
            t = self.tensor(name)
            if t is not None:
                out[name] = t[b, :n].cpu().numpy().copy()
        return out


# ---- intensity feature extraction (sensor_processing/feature_extractors) ----
SELECT_CANONICAL, SELECT_LIBSTDCXX = 0, 1
BF_DENSE_POPCOUNT, BF_DENSE_MATRIX_WHEN_FULL, BF_DENSE_MATRIX = 0, 1, 2  # include/proslam_hip.h PRS_BF_DENSE_*


def extractor_params(threshold=15, nms=1, target=1000, vertical=3, horizontal=3, selection_order=SELECT_CANONICAL, max_raw_detections=0):
    """defaults of configurations/kitti.conf:229-255.  selection_order: tie handling of the per-region cut
    (SELECT_LIBSTDCXX = GNU std::sort's permutation, what a GCC build of the reference does; slower);
    max_raw_detections: FAST detections per image the selection holds (0 = 8192, at most 32768)"""
    return _lib.ExtractorParams(threshold, nms, target, vertical, horizontal, selection_order, max_raw_detections)


def extract_features(ctx, params, image, capacity=4096):
    """host arrays, one 8-bit image [rows, cols] -> (uv [n, 2] f32, intensity [n] f32, descriptors [n, 32] u8); synchronises"""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    rows, cols = img.shape
    uv = np.zeros((capacity, 2), dtype=np.float32)
    inten = np.zeros(capacity, dtype=np.float32)
    desc = np.zeros((capacity, 32), dtype=np.uint8)
    n = C.c_int32(0)
    rc = _lib.load().prs_extract_features(ctx._h, C.byref(params), _p(img), rows, cols, cols, _p(uv), _p(inten), _p(desc), capacity, C.byref(n))
    _check(ctx, rc, "prs_extract_features")
    k = n.value
    return uv[:k].copy(), inten[:k].copy(), desc[:k].copy()


# ---- selective extraction (IntensityFeatureExtractorSelective_, GFTT corners around the projections of tracked landmarks) ----
DETECTOR_GFTT, DETECTOR_FAST = 0, 1            # PRS_DETECTOR_* (FAST is not built: PRS_ERR_UNSUPPORTED)
DESCRIPTOR_ORB_256, DESCRIPTOR_BRIEF_256 = 0, 1  # PRS_DESCRIPTOR_* (both cv::ORB in the reference's build)
_DETECTORS = {"GFTT": DETECTOR_GFTT, "FAST": DETECTOR_FAST}
_DESCRIPTORS = {"ORB-256": DESCRIPTOR_ORB_256, "BRIEF-256": DESCRIPTOR_BRIEF_256}


def selective_extractor_params(detector_type="GFTT", descriptor_type="ORB-256", target_number_of_keypoints=1000,
                               target_bin_width_pixels=10, enable_full_distance_to_left=False, enable_full_distance_to_right=False,
                               enable_seeding_when_tracking=True, max_candidates=0):
    """prs_selective_extractor_params; types by the reference's PARAM strings or the PRS_* values.  max_candidates: GFTT
    candidates per run the selection sort holds (0 = 8192, at most 16384)"""
    det = _DETECTORS[detector_type] if isinstance(detector_type, str) else int(detector_type)
    desc = _DESCRIPTORS[descriptor_type] if isinstance(descriptor_type, str) else int(descriptor_type)
    return _lib.SelectiveExtractorParams(det, desc, int(target_number_of_keypoints), int(target_bin_width_pixels),
                                         int(bool(enable_full_distance_to_left)), int(bool(enable_full_distance_to_right)),
                                         int(bool(enable_seeding_when_tracking)), int(max_candidates))


def extract_features_selective(ctx, params, image, projections=None, radius=0, capacity=4096, seeding_mask=None):
    """host arrays, one 8-bit image [rows, cols]; projections [n, 2] (u, v) = tracking mode, None / empty = seeding mode
    (seeding_mask [rows, cols], non-zero = detect, applies there only) -> (uv [n, 2] f32, intensity [n] f32,
    descriptors [n, 32] u8); synchronises"""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    rows, cols = img.shape
    proj = None if projections is None else np.ascontiguousarray(projections, dtype=np.float32).reshape(-1, 2)
    n_proj = 0 if proj is None else len(proj)
    mask = None if seeding_mask is None else np.ascontiguousarray(seeding_mask, dtype=np.uint8)
    if mask is not None and mask.shape != img.shape:
        raise ValueError("seeding_mask must have the image's shape")
    uv = np.zeros((capacity, 2), dtype=np.float32)
    inten = np.zeros(capacity, dtype=np.float32)
    desc = np.zeros((capacity, 32), dtype=np.uint8)
    n = C.c_int32(0)
    rc = _lib.load().prs_extract_features_selective(ctx._h, C.byref(params), _p(img), rows, cols, cols, _p(proj) if n_proj else None, n_proj,
                                                    int(radius), _p(mask) if mask is not None else None, _p(uv), _p(inten), _p(desc),
                                                    capacity, C.byref(n))
    _check(ctx, rc, "prs_extract_features_selective")
    k = n.value
    return uv[:k].copy(), inten[:k].copy(), desc[:k].copy()


def extract_features_selective_batch(ctx, params, images, keypoints, descriptors, n_features, status, intensity=None,
                                     projections=None, n_projections=None, radius=None, seeding_mask=None):
    """images: uint8 device tensor [B, rows, cols(pitch)]; projections: f32 device tensor [B, P, 2] with n_projections
    (i32 [B]; 0 = that image seeds) and radius (i32 [B] or None = 0); seeding_mask: uint8 device tensor shaped like images,
    or None.  Outputs as extract_features_batch."""
    d = _lib.SelectiveExtractBatch()
    d.batch, d.rows, d.cols, d.pitch = int(images.shape[0]), int(images.shape[1]), int(images.shape[2]), int(images.stride(1))
    d.images = images.data_ptr()
    if projections is not None:
        d.projection_stride = int(projections.shape[1])
        d.projections, d.n_projections = projections.data_ptr(), n_projections.data_ptr()
    d.detection_radius = radius.data_ptr() if radius is not None else None
    if seeding_mask is not None:
        if tuple(seeding_mask.shape) != tuple(images.shape) or seeding_mask.stride(1) != images.stride(1):
            raise ValueError("seeding_mask must have the images' shape and pitch")
        d.seeding_mask = seeding_mask.data_ptr()
    d.stride = int(keypoints.shape[1])
    d.keypoints, d.descriptors = keypoints.data_ptr(), descriptors.data_ptr()
    d.intensity = intensity.data_ptr() if intensity is not None else None
    d.n_features, d.status = n_features.data_ptr(), status.data_ptr()
    return _run(ctx, "prs_extract_features_selective_batch", C.byref(params), C.byref(d))


def selftest_reciprocal(ctx):
    """(operands that differ from 1.0f / x, operands that took the short form) over all 2^32 float bit patterns (prs_selftest_reciprocal)"""
    counts = np.zeros(2, dtype=np.uint64)
    rc = _lib.load().prs_selftest_reciprocal(ctx._h, _p(counts))
    _check(ctx, rc, "prs_selftest_reciprocal")
    return int(counts[0]), int(counts[1])


def selection_order(ctx, response):
    """responses (1..255) of one region's keypoints in detection order -> the permutation the reference's std::sort leaves
    (order[k] = keypoint at position k; intensity_feature_extractor_binned.cpp:182-186); host arrays, synchronises"""
    r = np.ascontiguousarray(response, dtype=np.uint8)
    order = np.zeros(len(r), dtype=np.int32)
    rc = _lib.load().prs_selection_order(ctx._h, _p(r), len(r), _p(order))
    _check(ctx, rc, "prs_selection_order")
    return order


def extract_features_batch(ctx, params, images, keypoints, descriptors, n_features, status, intensity=None):
    """images: uint8 device tensor [B, rows, cols(pitch)]; outputs are device tensors laid out like the stereo
    matcher's inputs (keypoints [B, stride, 2] f32, descriptors [B, stride, 32] u8, n_features [B] i32)."""
    d = _lib.ExtractBatch()
    d.batch, d.rows, d.cols, d.pitch = int(images.shape[0]), int(images.shape[1]), int(images.shape[2]), int(images.stride(1))
    d.images = images.data_ptr()
    d.stride = int(keypoints.shape[1])
    d.keypoints, d.descriptors = keypoints.data_ptr(), descriptors.data_ptr()
    d.intensity = intensity.data_ptr() if intensity is not None else None
    d.n_features, d.status = n_features.data_ptr(), status.data_ptr()
    return _run(ctx, "prs_extract_features_batch", C.byref(params), C.byref(d))


# ---- RGB-D preprocessing (RawDataPreprocessorMonocularDepth: extractor keypoints + depth image -> (u, v, d) measurements) ----
DEPTH_U16, DEPTH_F32 = 0, 1  # PRS_DEPTH_* (TYPE_16UC1 / TYPE_32FC1)
_DEPTH_TYPES = {"u16": DEPTH_U16, "f32": DEPTH_F32}
_DEPTH_NP = {DEPTH_U16: np.uint16, DEPTH_F32: np.float32}


def depth_params(depth_type="u16", scale=1.0):
    """prs_depth_params; depth_type "u16" / "f32" or a PRS_DEPTH_* value, scale = depth_scaling_factor_to_meters
    (raw_data_preprocessor_monocular_depth.h:26-30, default 1.0; icl.conf:646 / tum.conf:638 use 0.001)"""
    t = _DEPTH_TYPES[depth_type] if isinstance(depth_type, str) else int(depth_type)
    return _lib.DepthParams(t, float(scale))


def depth_measurements(ctx, params, depth, keypoints, descriptors, intensity=None):
    """host arrays, one image: depth [rows, cols] (uint16 or float32 as params.depth_type), keypoints [n, 2] (u, v),
    descriptors [n, 32], intensity [n] or None -> (uvd [k, 3] f32, intensity [k] f32 or None, descriptors [k, 32] u8, status);
    synchronises"""
    dep = np.ascontiguousarray(depth, dtype=_DEPTH_NP.get(params.depth_type))  # an unknown type is the library's to refuse
    rows, cols = dep.shape
    kp = _np(keypoints, np.float32, (-1, 2))
    n = kp.shape[0]
    desc = _np(descriptors, np.uint8, (n, 32))
    inten = None if intensity is None else _np(intensity, np.float32, (n,))
    cap = max(n, 1)
    uvd = np.zeros((cap, 3), dtype=np.float32)
    inten_out = np.zeros(cap, dtype=np.float32)
    desc_out = np.zeros((cap, 32), dtype=np.uint8)
    k = C.c_int32(0)
    rc = _lib.load().prs_depth_measurements(ctx._h, C.byref(params), _p(dep), rows, cols, dep.strides[0], _p(kp),
                                            _p(inten) if inten is not None else None, _p(desc), n, _p(uvd), _p(inten_out), _p(desc_out),
                                            C.byref(k))
    _check(ctx, rc, "prs_depth_measurements")
    m = k.value
    return uvd[:m].copy(), (inten_out[:m].copy() if inten is not None else None), desc_out[:m].copy(), rc


def depth_measurements_batch(ctx, params, depth, keypoints, descriptors, n_features, fixed, fixed_desc, n_fixed, status,
                             intensity=None, fixed_intensity=None, extract_status=None):
    """device tensors: depth [B, rows, cols(pitch)] uint16 / float32; keypoints [B, stride, 2] f32, descriptors [B, stride, 32] u8,
    n_features [B] i32 (an extractor's outputs), intensity [B, stride] f32 or None, extract_status [B] i32 or None (may be
    `status`); out: fixed [B, stride, 4] f32 (u, v, d, 0), fixed_desc [B, stride, 32] u8, fixed_intensity [B, stride] f32 (with
    intensity), n_fixed [B] i32, status [B] i32.  Enqueues on the context stream (asynchronous)."""
    d = _lib.DepthBatch()
    d.batch, d.rows, d.cols = int(depth.shape[0]), int(depth.shape[1]), int(depth.shape[2])
    d.pitch = int(depth.stride(1)) * depth.element_size()
    d.depth = depth.data_ptr()
    d.stride = int(keypoints.shape[1])
    for t in (descriptors, fixed, fixed_desc) + ((intensity, fixed_intensity) if intensity is not None else ()):
        if int(t.shape[1]) != d.stride:
            raise ValueError("every per-feature tensor needs the keypoints' stride")
    d.keypoints, d.descriptors, d.n_features = keypoints.data_ptr(), descriptors.data_ptr(), n_features.data_ptr()
    d.intensity = intensity.data_ptr() if intensity is not None else None
    d.extract_status = extract_status.data_ptr() if extract_status is not None else None
    d.fixed, d.fixed_desc, d.n_fixed, d.status = fixed.data_ptr(), fixed_desc.data_ptr(), n_fixed.data_ptr(), status.data_ptr()
    d.fixed_intensity = fixed_intensity.data_ptr() if fixed_intensity is not None else None
    return _run(ctx, "prs_depth_measurements_batch", C.byref(params), C.byref(d))


class RGBDFrames:
    """B RGB-D frames resident in HBM: the intensity and depth images, the extractor's outputs and the depth stage's
    measurements.  `fixed` / `fixed_desc` / `n_fixed` have the layout of AlignFrames.fixed / fixed_desc / n_fixed and
    MapBatch.measurement / measurement_desc / n_measured, so those can point at them (as StereoFrames.fixed_uvuv does for stereo):
    extract -> depth -> align / merge without a host copy.  `status` holds the extractor's status after extract() and the
    depth stage's after depth()."""

    def __init__(self, device, batch, rows, cols, stride, depth_type="u16", with_intensity=True):
        import torch
        dev = torch.device("cuda", device)
        self.batch, self.rows, self.cols, self.stride = int(batch), int(rows), int(cols), int(stride)
        t = _DEPTH_TYPES[depth_type] if isinstance(depth_type, str) else int(depth_type)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.images = z((batch, rows, cols), torch.uint8)
        self.depth = z((batch, rows, cols), torch.uint16 if t == DEPTH_U16 else torch.float32)
        self.keypoints = z((batch, stride, 2), torch.float32)
        self.descriptors = z((batch, stride, 32), torch.uint8)
        self.intensity = z((batch, stride), torch.float32) if with_intensity else None
        self.n_features = z((batch,), torch.int32)
        self.fixed = z((batch, stride, 4), torch.float32)
        self.fixed_desc = z((batch, stride, 32), torch.uint8)
        self.fixed_intensity = z((batch, stride), torch.float32) if with_intensity else None
        self.n_fixed = z((batch,), torch.int32)
        self.status = z((batch,), torch.int32)

    def upload(self, b, image, depth):
        import torch
        self.images[b] = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8))
        self.depth[b] = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.uint16 if self.depth.dtype == torch.uint16 else np.float32))

    def extract(self, ctx, extractor_params_):
        """the binned extractor on every image (status <- the extractor's)"""
        return extract_features_batch(ctx, extractor_params_, self.images, self.keypoints, self.descriptors, self.n_features,
                                      self.status, self.intensity)

    def measure(self, ctx, depth_params_):
        """the depth stage on the extractor's outputs in place (status <- the extractor's error or the stage's own)"""
        return depth_measurements_batch(ctx, depth_params_, self.depth, self.keypoints, self.descriptors, self.n_features, self.fixed,
                                        self.fixed_desc, self.n_fixed, self.status, self.intensity, self.fixed_intensity, self.status)

    def run(self, ctx, extractor_params_, depth_params_):
        self.extract(ctx, extractor_params_)
        return self.measure(ctx, depth_params_)

    def fixed_of(self, b):
        """download frame b: (uvd [k, 3] f32, descriptors [k, 32] u8, intensity [k] f32 or None, status)"""
        k = int(self.n_fixed[b].item())
        uvd = self.fixed[b, :k, :3].cpu().numpy().copy()
        desc = self.fixed_desc[b, :k].cpu().numpy().copy()
        inten = self.fixed_intensity[b, :k].cpu().numpy().copy() if self.fixed_intensity is not None else None
        return uvd, desc, inten, int(self.status[b].item())


def rgbd_params(cfg, selection_order=SELECT_LIBSTDCXX, max_raw_detections=32768, depth_type="u16"):
    """(prs_extractor_params, prs_depth_params) of a configs.* RGB-D dictionary's "rgbd" group (icl, tum); the extractor keeps the
    reference's std::sort order by default"""
    r = cfg["rgbd"]
    ep = extractor_params(int(r["detector_threshold"]), int(r["enable_non_maximum_suppression"]), int(r["target_number_of_keypoints"]),
                          int(r["number_of_detectors_vertical"]), int(r["number_of_detectors_horizontal"]), selection_order, max_raw_detections)
    return ep, depth_params(depth_type, r["depth_scaling_factor_to_meters"])


# ---- what the adapters of the image stages share: each [batch][frames][rows][cols] stage below states only what is its own ----
def _depth_type(depth_type, known=False):
    """PRS_DEPTH_* of "u16" / "f32" or of an integer, which goes to the library as it is unless it has to be a known one"""
    if depth_type not in _DEPTH_TYPES if isinstance(depth_type, str) else known and int(depth_type) not in _DEPTH_TYPES.values():
        raise ValueError("depth_type: one of %s" % (sorted(_DEPTH_TYPES),))
    return _DEPTH_TYPES[depth_type] if isinstance(depth_type, str) else int(depth_type)


def _zeros_on(device):
    """zeros(shape, dtype) on a device: an index is that GPU, a torch.device itself"""
    import torch
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    return lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)


def _padded_rows(z, lead, cols, dtype, wanted=True):
    """(storage, view, pitch in elements) of an array [*lead, cols] whose rows are padded to a multiple of four elements; the view
    has the cols columns.  Not wanted: (None, None, pitch)"""
    padded = (cols + 3) // 4 * 4
    storage = z(tuple(lead) + (padded,), dtype) if wanted else None
    return storage, (storage[..., :cols] if wanted else None), padded


def _subset(outputs, known):
    if set(outputs) - set(known):
        raise ValueError("outputs: a subset of %s" % (known,))


def _follow(t, rows, strict=False):
    """whether the images of t, [..., rows, cols], follow one another at rows * pitch; a dimension of length 1 may have any stride
    unless strict"""
    step, dense = rows * int(t.stride(-2)), True
    for n, stride in zip(t.shape[-3::-1], t.stride()[-3::-1]):
        dense = dense and ((n == 1 and not strict) or int(stride) == step)
        step *= int(n)
    return dense


def _images(t, name, dtype, shape, type_name=None, in_bytes=False):
    """(pointer, pitch in elements or in bytes) of a tensor of this dtype, shape = [B, frames, rows, cols] or [B * frames, rows,
    cols], whose images follow one another at rows * pitch (a pitch above cols is allowed)"""
    B, F, rows, cols = shape
    if t.dtype != dtype or t.stride(-1) != 1 or tuple(t.shape) not in ((B, F, rows, cols), (B * F, rows, cols)):
        raise ValueError("%s must be a %s tensor [%d, %d, %d, %d] or [%d, %d, %d] with contiguous rows" % (name, type_name or dtype, B, F, rows, cols, B * F, rows, cols))
    if int(t.stride(-2)) < cols or not _follow(t, rows):
        raise ValueError("the images of %s must follow one another at rows * pitch" % name)
    return t.data_ptr(), int(t.stride(-2)) * (t.element_size() if in_bytes else 1)


def _int32_ptr(t, name, shape, any_type=False):
    """the pointer of an optional contiguous int32 tensor of this shape (None stays None); any_type: its type is not looked at"""
    import torch
    if t is None:
        return None
    if tuple(t.shape) != tuple(shape) or not (any_type or t.dtype == torch.int32) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s[%s]" % (name, "" if any_type else "int32 tensor ", ", ".join("%d" % n for n in shape)))
    return t.data_ptr()


def _n_images_ptr(n_images, batch):
    """n_images must be a contiguous int32 tensor [batch], or None: every sequence has `frames` images"""
    return _int32_ptr(n_images, "n_images", (batch,))


def _stereo_common(p, camera, n_disparities, min_disparity, uniqueness_percent, lr_max_diff):
    """the fields and the refusals that prs_dense_stereo_params and prs_sgm_stereo_params share; bf = float32(float64(fx) *
    float64(baseline_m))"""
    p.n_disparities, p.min_disparity, p.uniqueness_percent, p.lr_max_diff = int(n_disparities), int(min_disparity), int(uniqueness_percent), int(lr_max_diff)
    with np.errstate(over="ignore"):  # a product beyond float32 becomes inf and is refused below
        p.bf = float(np.float32(np.float64(camera["fx"]) * np.float64(camera["baseline_m"])))
    if not 1 <= p.n_disparities <= 256:
        raise ValueError("n_disparities must lie in 1 .. 256")
    if p.min_disparity < 0 or p.min_disparity + p.n_disparities > 4096:
        raise ValueError("min_disparity must be at least 0 and min_disparity + n_disparities at most 4096")
    if not 0 <= p.uniqueness_percent <= 99:
        raise ValueError("uniqueness_percent must lie in 0 .. 99")
    if not -1 <= p.lr_max_diff <= 255:
        raise ValueError("lr_max_diff must lie in -1 .. 255")
    if not (np.isfinite(p.bf) and p.bf > 0.0):
        raise ValueError("fx * baseline_m must be finite and positive as a float32")
    return p


# ---- dense RGB-D cloud: the depth pixels of a sequence's frames in the world frame (include/proslam_hip.h prs_depth_cloud_*) ----
def depth_cloud_params(camera, range_min=0.1, range_max=10.0, step=1, depth_type="u16", scale=1.0, sensor_in_robot=None):
    """prs_depth_cloud_params.  camera: a dictionary with fx, fy, cx, cy (configs.*["camera"]); range_min / range_max in metres
    (the defaults of the reference's unprojection app); step: the pixel stride in both directions; depth_type "u16" / "f32" or a
    PRS_DEPTH_* value; scale = depth_scaling_factor_to_meters (1e-3 for the 16-bit millimetre images of icl and tum);
    sensor_in_robot [4, 4] or 16 values, row-major (None: the identity, the poses are the camera's)"""
    p = _lib.DepthCloudParams()
    p.depth_type = _depth_type(depth_type)
    p.depth_scaling_factor_to_meters = float(scale)
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    p.range_min, p.range_max, p.step = float(range_min), float(range_max), int(step)
    S = np.eye(4, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(4, 4)
    p.sensor_in_robot[:] = [float(x) for x in S.reshape(16)]
    values = [p.depth_scaling_factor_to_meters, p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max] + list(p.sensor_in_robot)
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not p.depth_scaling_factor_to_meters > 0.0:
        raise ValueError("scale must be positive as a float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    if p.step < 1:
        raise ValueError("step must be at least 1")
    return p


class DepthCloudBatch:
    """the dense clouds of B sequences of up to `frames` depth images of rows x cols pixels: owns xyz (out_stride rows per
    sequence), the per-sequence counts and the workspace.  outputs: which of the optional arrays ("frame", "pixel") are kept; they
    are exposed as `node` and `row`, with n_opt = desc = None, so that WorldVoxelBatch.run(ctx, p, this) reads the cloud in place.
    The workspace is sized for step 1, which fits every step."""

    OPTIONAL = ("frame", "pixel")

    def __init__(self, batch, frames, rows, cols, out_stride, outputs=OPTIONAL, device=0):
        import torch
        _subset(outputs, self.OPTIONAL)
        B, F, n = int(batch), int(frames), int(out_stride)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1 or n < 1:
            raise ValueError("batch, frames, rows, cols and out_stride must be at least 1")
        self.batch, self.frames, self.rows, self.cols, self.out_stride = B, F, int(rows), int(cols), n
        z = _zeros_on(device)
        self.xyz = z((B, n, 4), torch.float32)
        self.node = z((B, n), torch.int32) if "frame" in outputs else None  # the image of a row, where a world map has the node
        self.row = z((B, n), torch.int32) if "pixel" in outputs else None   # v * cols + u, where a world map has the landmark's row
        self.n_opt, self.desc = None, None
        self.n_out, self.n_total, self.n_skipped = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.status = z((B,), torch.int32)
        nbytes = int(_lib.load().prs_depth_cloud_workspace_bytes(B, F, self.rows, self.cols, 1))
        if nbytes < 1:
            raise ValueError("frames * rows * cols must stay below 2^31")
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, depth, pose, n_images, frame_index=None, gray=None, append=False, count_only=False):
        """the prs_depth_cloud_batch of device tensors: depth [B, frames, rows, cols (or more: the pitch)] uint16 / float32, pose
        [B, pose_stride, 16] float32, n_images [B] int32, frame_index [B, frames] int32 or None, gray like depth, uint8, or None"""
        B, F = self.batch, self.frames
        if depth.dim() != 4 or tuple(depth.shape[:3]) != (B, F, self.rows) or int(depth.shape[3]) < self.cols or depth.stride(3) != 1:
            raise ValueError("depth must be [%d, %d, %d, >= %d] with contiguous rows" % (B, F, self.rows, self.cols))
        if not _follow(depth, self.rows, strict=True):
            raise ValueError("the images of depth must follow one another at rows * pitch")
        if pose.dim() != 3 or int(pose.shape[0]) != B or int(pose.shape[2]) != 16 or not pose.is_contiguous():
            raise ValueError("pose must be a contiguous [%d, pose_stride, 16]" % B)
        d = _lib.DepthCloudBatch()
        d.batch, d.frames, d.rows, d.cols, d.out_stride = B, F, self.rows, self.cols, self.out_stride
        d.pitch, d.pose_stride = int(depth.stride(2)) * depth.element_size(), int(pose.shape[1])
        d.depth, d.pose, d.n_images = depth.data_ptr(), pose.data_ptr(), n_images.data_ptr()
        if gray is not None:
            if tuple(gray.shape[:3]) != (B, F, self.rows) or int(gray.shape[3]) < self.cols or gray.stride(3) != 1 or \
                    not _follow(gray, self.rows, strict=True):
                raise ValueError("gray must be laid out like depth")
            d.gray, d.gray_pitch = gray.data_ptr(), int(gray.stride(2))
        d.frame_index = _int32_ptr(frame_index, "frame_index", (B, F), any_type=True)
        d.n_base = self.n_out.data_ptr() if append else None
        for name in ("n_out", "n_total", "n_skipped", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        if not count_only:
            d.xyz = self.xyz.data_ptr()
            d.frame = self.node.data_ptr() if self.node is not None else None
            d.pixel = self.row.data_ptr() if self.row is not None else None
        return d

    def _launch(self, ctx, params, d):
        return _run(ctx, "prs_depth_cloud_batch_run", C.byref(params), C.byref(d))

    def run(self, ctx, params, depth, pose, n_images, frame_index=None, gray=None, append=False):
        """enqueue the clouds of every sequence (asynchronous); per-sequence status lands in self.status.  append: the rows go behind
        the n_out rows an earlier call left, so a long sequence is fed chunk by chunk"""
        return self._launch(ctx, params, self.descriptor(depth, pose, n_images, frame_index, gray, append))

    def count(self, ctx, params, depth, pose, n_images, frame_index=None, gray=None, append=False):
        """enqueue the count-only call (asynchronous): n_total, n_skipped and status; n_out stays (append) or becomes 0"""
        return self._launch(ctx, params, self.descriptor(depth, pose, n_images, frame_index, gray, append, count_only=True))

    def cloud_of(self, b):
        """dict of numpy arrays trimmed to n_out rows, in the shape of WorldMapBatch.cloud_of (node is the image, row the pixel, bounds
        None) plus n_skipped; copies to the host when called"""
        n = min(max(int(self.n_out[b].item()), 0), self.out_stride)
        out = dict(n_out=n, n_total=int(self.n_total[b].item()), n_skipped=int(self.n_skipped[b].item()), n_nonfinite=0,
                   status=int(self.status[b].item()), xyz=self.xyz[b, :n].cpu().numpy().copy(), bounds=None)
        for name in ("node", "row"):
            t = getattr(self, name)
            if t is not None:
                out[name] = t[b, :n].cpu().numpy().copy()
        return out


# ---- dense stereo: rectified pairs to disparity and depth images (include/proslam_hip.h prs_dense_stereo_*) ----
def dense_stereo_params(camera, n_disparities=128, min_disparity=0, aggregation_radius=3, uniqueness_percent=10, lr_max_diff=1):
    """prs_dense_stereo_params.  camera: a dictionary with fx and baseline_m (configs.*["camera"], or the one ops.stereo_rectification
    returns); bf = float32(float64(fx) * float64(baseline_m)).  Disparities min_disparity .. min_disparity + n_disparities - 1, a box of
    (2 * aggregation_radius + 1)^2 census costs, uniqueness_percent 0 = no test, lr_max_diff -1 = no left-right check.  Raises
    ValueError on every value the library refuses"""
    p = _stereo_common(_lib.DenseStereoParams(), camera, n_disparities, min_disparity, uniqueness_percent, lr_max_diff)
    p.aggregation_radius = int(aggregation_radius)
    if not 0 <= p.aggregation_radius <= 7:
        raise ValueError("aggregation_radius must lie in 0 .. 7")
    return p


class DenseStereoBatch:
    """dense stereo of B sequences of up to `frames` rectified pairs of rows x cols pixels: owns the outputs named in `outputs`
    (disparity and depth [B, frames, rows, cols] float32 views of rows padded to a multiple of four floats, n_valid [B, frames]),
    status and the workspace, which is sized for the left-right check.  depth is what DepthCloudBatch.run takes with
    depth_type="f32" and scale 1."""

    OUTPUTS = ("disparity", "depth", "n_valid")

    def __init__(self, batch, frames, rows, cols, outputs=OUTPUTS, device=0):
        import torch
        _subset(outputs, self.OUTPUTS)
        if "disparity" not in outputs and "depth" not in outputs:
            raise ValueError("outputs: disparity, depth or both")
        B, F = int(batch), int(frames)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1:
            raise ValueError("batch, frames, rows and cols must be at least 1")
        self.batch, self.frames, self.rows, self.cols = B, F, int(rows), int(cols)
        z = _zeros_on(device)
        self._disparity, self.disparity, padded = _padded_rows(z, (B, F, self.rows), self.cols, torch.float32, "disparity" in outputs)
        self._depth, self.depth, padded = _padded_rows(z, (B, F, self.rows), self.cols, torch.float32, "depth" in outputs)
        self.out_pitch = padded * 4
        self.n_valid = z((B, F), torch.int32) if "n_valid" in outputs else None
        self.status = z((B,), torch.int32)
        nbytes = self._workspace_bytes()
        if nbytes < 1:
            raise ValueError("batch * frames * rows * cols must stay below 2^31")
        self.workspace = z((nbytes,), torch.uint8)

    def _workspace_bytes(self):
        return int(_lib.load().prs_dense_stereo_workspace_bytes(self.batch, self.frames, self.rows, self.cols, 1, 1))

    def descriptor(self, left, right, n_images=None):
        """the prs_dense_stereo_batch of device tensors: left, right uint8 [B, frames, rows, cols] or [B * frames, rows, cols] (the two
        halves of a RectifyBatch's dst, with their pitch), n_images [B] int32 or None = frames"""
        d = _lib.DenseStereoBatch()
        self._fill(d, left, right, n_images)
        return d

    def _fill(self, d, left, right, n_images):
        d.batch, d.frames, d.rows, d.cols, d.out_pitch = self.batch, self.frames, self.rows, self.cols, self.out_pitch
        import torch
        shape = (self.batch, self.frames, self.rows, self.cols)
        d.left, d.left_pitch = _images(left, "left", torch.uint8, shape, "uint8")
        d.right, d.right_pitch = _images(right, "right", torch.uint8, shape, "uint8")
        d.n_images = _n_images_ptr(n_images, self.batch)
        d.disparity = self._disparity.data_ptr() if self._disparity is not None else None
        d.depth = self._depth.data_ptr() if self._depth is not None else None
        d.n_valid = self.n_valid.data_ptr() if self.n_valid is not None else None
        d.status, d.workspace = self.status.data_ptr(), self.workspace.data_ptr()

    def run(self, ctx, params, left, right, n_images=None):
        """enqueue the disparity and depth images of every pair (asynchronous); per-sequence status lands in self.status"""
        d = self.descriptor(left, right, n_images)
        return _run(ctx, "prs_dense_stereo_batch_run", C.byref(params), C.byref(d))


# ---- semi-global dense stereo: rectified pairs to disparity and depth images by path aggregation (include/proslam_hip.h prs_sgm_stereo_*) ----
def sgm_stereo_params(camera, n_disparities=configs.SGM_STEREO["n_disparities"], min_disparity=configs.SGM_STEREO["min_disparity"],
                      p1=configs.SGM_STEREO["p1"], p2=configs.SGM_STEREO["p2"], n_paths=configs.SGM_STEREO["n_paths"],
                      uniqueness_percent=configs.SGM_STEREO["uniqueness_percent"], lr_max_diff=configs.SGM_STEREO["lr_max_diff"]):
    """prs_sgm_stereo_params.  camera: a dictionary with fx and baseline_m, as ops.dense_stereo_params takes it.  Disparities
    min_disparity .. min_disparity + n_disparities - 1, the penalties 0 <= p1 <= p2 <= 4095 of a path's step of one disparity and of a
    larger one, n_paths 4 or 8, uniqueness_percent 0 = no test, lr_max_diff -1 = no left-right check.  The defaults are
    configs.SGM_STEREO (128, 0, 10, 120, 8, 10, 1).  Raises ValueError on every value the library refuses"""
    p = _stereo_common(_lib.SgmStereoParams(), camera, n_disparities, min_disparity, uniqueness_percent, lr_max_diff)
    p.p1, p.p2, p.n_paths = int(p1), int(p2), int(n_paths)
    if not 0 <= p.p1 <= p.p2 <= 4095:
        raise ValueError("the penalties must satisfy 0 <= p1 <= p2 <= 4095")
    if p.n_paths not in (4, 8):
        raise ValueError("n_paths must be 4 or 8")
    return p


def sgm_stereo_images_in_flight(batch, frames, rows, cols, n_disparities=256):
    """the images_in_flight SgmStereoBatch picks when it is left to it: the largest count whose S volumes (2 * rows * cols *
    n_disparities bytes an image) stay within configs.SGM_STEREO_VOLUME_BUDGET, at least 1 and at most batch * frames"""
    volume = 2 * int(rows) * int(cols) * int(n_disparities)
    return max(1, min(int(batch) * int(frames), configs.SGM_STEREO_VOLUME_BUDGET // volume))


class SgmStereoBatch(DenseStereoBatch):
    """semi-global dense stereo of B sequences of up to `frames` rectified pairs of rows x cols pixels: the outputs, padding,
    out_pitch and run signature of DenseStereoBatch, so SpeckleFilterBatch and DepthCloudBatch read disparity and depth in place.
    The workspace is sized for the left-right check, for params of up to `n_disparities` disparities and for the S volumes of
    `images_in_flight` images at a time; None picks ops.sgm_stereo_images_in_flight(...)."""

    def __init__(self, batch, frames, rows, cols, outputs=DenseStereoBatch.OUTPUTS, images_in_flight=None, n_disparities=256, device=0):
        self.n_disparities = int(n_disparities)
        if not 1 <= self.n_disparities <= 256:
            raise ValueError("n_disparities must lie in 1 .. 256")
        if images_in_flight is not None and int(images_in_flight) < 1:
            raise ValueError("images_in_flight must be at least 1")
        self._in_flight = None if images_in_flight is None else int(images_in_flight)
        super().__init__(batch, frames, rows, cols, outputs, device)

    def _workspace_bytes(self):
        if self._in_flight is None:
            self._in_flight = sgm_stereo_images_in_flight(self.batch, self.frames, self.rows, self.cols, self.n_disparities)
        self.images_in_flight = min(self._in_flight, self.batch * self.frames)
        return int(_lib.load().prs_sgm_stereo_workspace_bytes(self.batch, self.frames, self.rows, self.cols, self.n_disparities, 1,
                                                              self.images_in_flight))

    def descriptor(self, left, right, n_images=None):
        """the prs_sgm_stereo_batch of device tensors, as DenseStereoBatch.descriptor takes them"""
        d = _lib.SgmStereoBatch()
        self._fill(d, left, right, n_images)
        d.images_in_flight = self.images_in_flight
        return d

    def run(self, ctx, params, left, right, n_images=None):
        """enqueue the disparity and depth images of every pair (asynchronous); per-sequence status lands in self.status"""
        if params.n_disparities > self.n_disparities:
            raise ValueError("the workspace was sized for %d disparities, the params have %d" % (self.n_disparities, params.n_disparities))
        d = self.descriptor(left, right, n_images)
        return _run(ctx, "prs_sgm_stereo_batch_run", C.byref(params), C.byref(d))


# ---- speckle filter: the small segments of a disparity or depth image set to 0 in place (include/proslam_hip.h prs_speckle_*) ----
def speckle_params(max_size=200, max_diff=1.0, pixel_type="f32", companion_type=None):
    """prs_speckle_params.  Components of at most max_size pixels are removed (0: none); 4-neighbours are connected when both are
    > 0 and differ by at most max_diff as float32 (the defaults are configs.SPECKLE); pixel_type "f32" / "u16" of the image,
    companion_type of the companion image (None: pixel_type; read only when SpeckleFilterBatch.run is given a companion).  Raises
    ValueError on every value the library refuses"""
    types = {"u16": PIXEL_U16, "f32": PIXEL_F32}
    if pixel_type not in types or (companion_type is not None and companion_type not in types):
        raise ValueError("pixel_type and companion_type: one of %s" % (sorted(types),))
    p = _lib.SpeckleParams()
    p.pixel_type = types[pixel_type]
    p.companion_type = p.pixel_type if companion_type is None else types[companion_type]
    if int(max_size) != max_size or not 0 <= int(max_size) <= 0x7fffffff:
        raise ValueError("max_size must be an integer in 0 .. 2^31 - 1")
    p.max_size = int(max_size)
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.max_diff = float(np.float32(max_diff))
    if not (np.isfinite(p.max_diff) and p.max_diff >= 0.0):
        raise ValueError("max_diff must be finite as a float32 and at least 0")
    return p


class SpeckleFilterBatch:
    """the speckle filter of B sequences of up to `frames` images of rows x cols pixels, in place: owns the outputs named in `outputs`
    (n_kept and n_removed [B, frames]; label [B, frames, rows, cols] int32, a view of rows padded to a multiple of four), status and
    the workspace.  A DenseStereoBatch's disparity with its depth as the companion, or a RectifyBatch's 16-bit depth, go in as they
    are; what comes out is what DepthCloudBatch.run takes."""

    OUTPUTS = ("label", "n_kept", "n_removed")

    def __init__(self, batch, frames, rows, cols, outputs=("n_kept", "n_removed"), device=0):
        import torch
        _subset(outputs, self.OUTPUTS)
        B, F = int(batch), int(frames)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1:
            raise ValueError("batch, frames, rows and cols must be at least 1")
        self.batch, self.frames, self.rows, self.cols = B, F, int(rows), int(cols)
        z = _zeros_on(device)
        self._label, self.label, padded = _padded_rows(z, (B, F, self.rows), self.cols, torch.int32, "label" in outputs)
        self.label_pitch = padded * 4
        self.n_kept = z((B, F), torch.int32) if "n_kept" in outputs else None
        self.n_removed = z((B, F), torch.int32) if "n_removed" in outputs else None
        self.status = z((B,), torch.int32)
        nbytes = int(_lib.load().prs_speckle_workspace_bytes(B, F, self.rows, self.cols))
        if nbytes < 1:
            raise ValueError("rows * cols and batch * frames * rows * cols must stay below 2^31")
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, params, image, companion=None, n_images=None):
        """the prs_speckle_batch of device tensors: image (and companion) of params' pixel types, n_images [B] int32 or None = frames"""
        d = _lib.SpeckleBatch()
        d.batch, d.frames, d.rows, d.cols = self.batch, self.frames, self.rows, self.cols
        import torch
        types, shape = {PIXEL_U16: torch.uint16, PIXEL_F32: torch.float32}, (self.batch, self.frames, self.rows, self.cols)
        d.image, d.pitch = _images(image, "image", types[params.pixel_type], shape, in_bytes=True)
        if companion is not None:
            d.companion, d.companion_pitch = _images(companion, "companion", types[params.companion_type], shape, in_bytes=True)
        d.n_images = _n_images_ptr(n_images, self.batch)
        if self._label is not None:
            d.label, d.label_pitch = self._label.data_ptr(), self.label_pitch
        d.n_kept = self.n_kept.data_ptr() if self.n_kept is not None else None
        d.n_removed = self.n_removed.data_ptr() if self.n_removed is not None else None
        d.status, d.workspace = self.status.data_ptr(), self.workspace.data_ptr()
        return d

    def run(self, ctx, params, image, companion=None, n_images=None):
        """enqueue the filter of every image, in place (asynchronous); per-sequence status lands in self.status"""
        d = self.descriptor(params, image, companion, n_images)
        return _run(ctx, "prs_speckle_batch_run", C.byref(params), C.byref(d))


# ---- depth consistency filter: depth pixels cross-checked against the neighbouring frames (include/proslam_hip.h prs_depth_consistency_*) ----
def depth_consistency_params(camera, window=2, stride=1, max_rel_diff=0.02, min_support=2, max_violation=1, range_min=0.1, range_max=10.0,
                             depth_type="u16", scale=1.0, sensor_in_robot=None):
    """prs_depth_consistency_params.  camera: a dictionary with fx, fy, cx, cy (configs.*["camera"]); window neighbours on each side,
    `stride` frames apart; a neighbour supports a pixel whose depth it sees within max_rel_diff (relative), and violates one it sees
    past; kept with at least min_support supports and at most max_violation violations (the defaults are
    configs.DEPTH_CONSISTENCY); range_min / range_max, depth_type, scale and sensor_in_robot as in depth_cloud_params.  Raises
    ValueError on every value the library refuses"""
    p = _lib.DepthConsistencyParams()
    p.depth_type = _depth_type(depth_type, known=True)
    for name, value, lo, hi in (("window", window, 1, 8), ("stride", stride, 1, 0x7fffffff), ("min_support", min_support, 0, 16),
                                ("max_violation", max_violation, 0, 16)):
        if int(value) != value or not lo <= int(value) <= hi:
            raise ValueError("%s must be an integer in %d .. %d" % (name, lo, hi))
    p.window, p.stride, p.min_support, p.max_violation = int(window), int(stride), int(min_support), int(max_violation)
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.max_rel_diff = float(np.float32(max_rel_diff))
    if not (np.isfinite(p.max_rel_diff) and p.max_rel_diff >= 0.0):
        raise ValueError("max_rel_diff must be finite as a float32 and at least 0")
    p.depth_scaling_factor_to_meters = float(scale)
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    p.range_min, p.range_max = float(range_min), float(range_max)
    S = np.eye(4, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(4, 4)
    p.sensor_in_robot[:] = [float(x) for x in S.reshape(16)]
    values = [p.depth_scaling_factor_to_meters, p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max] + list(p.sensor_in_robot)
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not p.depth_scaling_factor_to_meters > 0.0:
        raise ValueError("scale must be positive as a float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    return p


class DepthConsistencyBatch:
    """the depth consistency filter of B sequences of up to `frames` depth images of rows x cols pixels with up to `window`
    neighbours on each side: owns out, the outputs named in `outputs` (support and violation [B, frames, rows, cols] uint8, n_kept
    and n_removed [B, frames], n_skipped [B]), status and the workspace.  out, support and violation are views of rows padded to a
    multiple of four elements; out is what DepthCloudBatch.run takes in place of the depth it was filtered from."""

    OUTPUTS = ("support", "violation", "n_kept", "n_removed", "n_skipped")

    def __init__(self, batch, frames, rows, cols, window, depth_type="u16", outputs=("n_kept", "n_removed"), device=0):
        import torch
        _subset(outputs, self.OUTPUTS)
        self.depth_type = _depth_type(depth_type, known=True)
        B, F = int(batch), int(frames)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1:
            raise ValueError("batch, frames, rows and cols must be at least 1")
        if not 1 <= int(window) <= 8:
            raise ValueError("window must lie in 1 .. 8")
        self.batch, self.frames, self.rows, self.cols, self.window = B, F, int(rows), int(cols), int(window)
        self.dtype = torch.uint16 if self.depth_type == DEPTH_U16 else torch.float32
        z = _zeros_on(device)
        self._out, self.out, _ = _padded_rows(z, (B, F, self.rows), self.cols, self.dtype)
        self._support, self.support, _ = _padded_rows(z, (B, F, self.rows), self.cols, torch.uint8, "support" in outputs)
        self._violation, self.violation, _ = _padded_rows(z, (B, F, self.rows), self.cols, torch.uint8, "violation" in outputs)
        self.n_kept = z((B, F), torch.int32) if "n_kept" in outputs else None
        self.n_removed = z((B, F), torch.int32) if "n_removed" in outputs else None
        self.n_skipped = z((B,), torch.int32) if "n_skipped" in outputs else None
        self.status = z((B,), torch.int32)
        nbytes = int(_lib.load().prs_depth_consistency_workspace_bytes(B, F, self.window))
        if nbytes < 1:
            raise ValueError("no workspace for these sizes")
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, depth, pose, n_images=None, frame_index=None):
        """the prs_depth_consistency_batch of device tensors: depth [B, frames, rows, cols (a view of longer rows is allowed: the
        pitch)] of the depth type, pose [B, pose_stride, 16] float32, n_images [B] int32 or None = frames, frame_index [B, frames]
        int32 or None"""
        B, F = self.batch, self.frames
        if depth.dtype != self.dtype or depth.dim() != 4 or tuple(depth.shape[:3]) != (B, F, self.rows) or int(depth.shape[3]) < self.cols or \
                depth.stride(3) != 1:
            raise ValueError("depth must be a %s tensor [%d, %d, %d, >= %d] with contiguous rows" % (self.dtype, B, F, self.rows, self.cols))
        if not _follow(depth, self.rows, strict=True):
            raise ValueError("the images of depth must follow one another at rows * pitch")
        if pose.dim() != 3 or int(pose.shape[0]) != B or int(pose.shape[2]) != 16 or not pose.is_contiguous():
            raise ValueError("pose must be a contiguous [%d, pose_stride, 16]" % B)
        d = _lib.DepthConsistencyBatch()
        d.batch, d.frames, d.rows, d.cols = B, F, self.rows, self.cols
        es = depth.element_size()
        d.pitch, d.out_pitch, d.count_pitch = int(depth.stride(2)) * es, int(self._out.stride(2)) * es, int(self._out.stride(2))
        d.pose_stride = int(pose.shape[1])
        d.depth, d.pose, d.out = depth.data_ptr(), pose.data_ptr(), self._out.data_ptr()
        d.n_images = _n_images_ptr(n_images, B)
        d.frame_index = _int32_ptr(frame_index, "frame_index", (B, F))
        for name, t in (("support", self._support), ("violation", self._violation), ("n_kept", self.n_kept), ("n_removed", self.n_removed),
                        ("n_skipped", self.n_skipped)):
            setattr(d, name, t.data_ptr() if t is not None else None)
        d.status, d.workspace = self.status.data_ptr(), self.workspace.data_ptr()
        return d

    def run(self, ctx, params, depth, pose, n_images=None, frame_index=None):
        """enqueue the filter of every image (asynchronous) and return out; per-sequence status lands in self.status.  params.window
        must not exceed the window the workspace was sized for"""
        if params.window > self.window:
            raise ValueError("params.window %d exceeds the window %d this batch was sized for" % (params.window, self.window))
        d = self.descriptor(depth, pose, n_images, frame_index)
        _run(ctx, "prs_depth_consistency_batch_run", C.byref(params), C.byref(d))
        return self.out


# ---- depth normals: depth images to oriented surface normals, per pixel and per cloud row (include/proslam_hip_normals.h) ----
def depth_normals_params(camera, radius=configs.DEPTH_NORMALS["radius"], smooth=configs.DEPTH_NORMALS["smooth"],
                         max_rel_diff=configs.DEPTH_NORMALS["max_rel_diff"], range_min=configs.DEPTH_NORMALS["range_min"],
                         range_max=configs.DEPTH_NORMALS["range_max"], depth_type="u16", scale=1.0, sensor_in_robot=None):
    """prs_depth_normals_params.  camera: a dictionary with fx, fy, cx, cy (configs.*["camera"]); the tangents reach `radius` pixels
    (1 .. 8) to each side, the raw normals are summed over a (2 smooth + 1)^2 window (smooth 0 .. 3, 0: none); a neighbour counts
    when its depth lies within max_rel_diff (relative) of the centre's; range_min / range_max, depth_type, scale and sensor_in_robot
    as in depth_cloud_params.  Raises ValueError on every value the library refuses"""
    p = _lib_normals.DepthNormalsParams()
    p.depth_type = _depth_type(depth_type, known=True)
    for name, value, lo, hi in (("radius", radius, 1, 8), ("smooth", smooth, 0, 3)):
        if int(value) != value or not lo <= int(value) <= hi:
            raise ValueError("%s must be an integer in %d .. %d" % (name, lo, hi))
    p.radius, p.smooth = int(radius), int(smooth)
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.max_rel_diff = float(np.float32(max_rel_diff))
    if not (np.isfinite(p.max_rel_diff) and p.max_rel_diff >= 0.0):
        raise ValueError("max_rel_diff must be finite as a float32 and at least 0")
    p.depth_scaling_factor_to_meters = float(scale)
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    p.range_min, p.range_max = float(range_min), float(range_max)
    S = np.eye(4, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(4, 4)
    p.sensor_in_robot[:] = [float(x) for x in S.reshape(16)]
    values = [p.depth_scaling_factor_to_meters, p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max] + list(p.sensor_in_robot)
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not p.depth_scaling_factor_to_meters > 0.0:
        raise ValueError("scale must be positive as a float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    return p


class DepthNormalsBatch:
    """the normals of B sequences of up to `frames` depth images of rows x cols pixels: owns normal [B, frames, rows, cols, 4]
    (n0, n1, n2, w in the camera frame), n_normal [B, frames] when "n_normal" is among `outputs`, and status.  With row_stride, the
    out_stride of an ops.DepthCloudBatch over the same images, it also owns row_normal [B, row_stride, 4], one world-frame normal per
    cloud row, n_bad_rows [B] and n_rows [B], the rows it has written so far."""

    OPTIONAL = ("n_normal",)

    def __init__(self, batch, frames, rows, cols, row_stride=None, outputs=OPTIONAL, device=0):
        import torch
        _subset(outputs, self.OPTIONAL)
        B, F = int(batch), int(frames)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1 or (row_stride is not None and int(row_stride) < 1):
            raise ValueError("batch, frames, rows, cols and row_stride must be at least 1")
        if B * F * int(rows) * int(cols) > 0x7fffffff:
            raise ValueError("batch * frames * rows * cols must stay below 2^31")
        _lib_normals.load()
        self.batch, self.frames, self.rows, self.cols = B, F, int(rows), int(cols)
        self.row_stride = None if row_stride is None else int(row_stride)
        z = _zeros_on(device)
        self.normal = z((B, F, self.rows, self.cols, 4), torch.float32)
        self.n_normal = z((B, F), torch.int32) if "n_normal" in outputs else None
        self.status = z((B,), torch.int32)
        with_rows = self.row_stride is not None
        self.row_normal = z((B, self.row_stride, 4), torch.float32) if with_rows else None
        self.n_bad_rows = z((B,), torch.int32) if with_rows else None
        self.n_rows = z((B,), torch.int32) if with_rows else None

    def descriptor(self, params, depth, pose=None, n_images=None, frame_index=None, cloud=None, append=False):
        """the prs_depth_normals_batch of device tensors: depth [B, frames, rows, cols (a view of longer rows is allowed: the
        pitch)] of params' depth type, n_images [B] int32 or None = frames, and with cloud (an ops.DepthCloudBatch that kept "frame"
        and "pixel", run on the same images) pose [B, pose_stride, 16] float32 and frame_index [B, frames] int32 or None"""
        import torch
        B, F = self.batch, self.frames
        dtype = torch.uint16 if params.depth_type == DEPTH_U16 else torch.float32
        if depth.dtype != dtype or depth.dim() != 4 or tuple(depth.shape[:3]) != (B, F, self.rows) or int(depth.shape[3]) < self.cols or \
                depth.stride(3) != 1:
            raise ValueError("depth must be a %s tensor [%d, %d, %d, >= %d] with contiguous rows" % (dtype, B, F, self.rows, self.cols))
        if not _follow(depth, self.rows, strict=True):
            raise ValueError("the images of depth must follow one another at rows * pitch")
        d = _lib_normals.DepthNormalsBatch()
        d.batch, d.frames, d.rows, d.cols = B, F, self.rows, self.cols
        d.pitch = int(depth.stride(2)) * depth.element_size()
        d.depth, d.normal, d.status = depth.data_ptr(), self.normal.data_ptr(), self.status.data_ptr()
        d.n_images = _n_images_ptr(n_images, B)
        d.n_normal = self.n_normal.data_ptr() if self.n_normal is not None else None
        if cloud is None:
            if append:
                raise ValueError("append needs a cloud")
            return d
        if self.row_stride is None:
            raise ValueError("this batch was built without row_stride: it has no rows for a cloud")
        if (cloud.batch, cloud.frames, cloud.rows, cloud.cols, cloud.out_stride) != (B, F, self.rows, self.cols, self.row_stride):
            raise ValueError("the cloud must have this batch's batch, frames, rows and cols, and row_stride as its out_stride")
        if cloud.node is None or cloud.row is None:
            raise ValueError('the cloud must keep its "frame" and "pixel" outputs')
        if pose is None or pose.dim() != 3 or int(pose.shape[0]) != B or int(pose.shape[2]) != 16 or pose.dtype != torch.float32 or \
                not pose.is_contiguous():
            raise ValueError("with a cloud, pose must be a contiguous float32 [%d, pose_stride, 16]" % B)
        d.pose, d.pose_stride, d.row_stride = pose.data_ptr(), int(pose.shape[1]), self.row_stride
        d.frame_index = _int32_ptr(frame_index, "frame_index", (B, F))
        d.row_frame, d.row_pixel, d.row_n = cloud.node.data_ptr(), cloud.row.data_ptr(), cloud.n_out.data_ptr()
        d.row_base = self.n_rows.data_ptr() if append else None
        d.row_normal, d.n_bad_rows = self.row_normal.data_ptr(), self.n_bad_rows.data_ptr()
        return d

    def run(self, ctx, params, depth, pose=None, n_images=None, frame_index=None, cloud=None, append=False):
        """enqueue the normals of every image (asynchronous) and return normal; per-sequence status lands in self.status.  cloud: the
        ops.DepthCloudBatch whose run on the same images and poses came before; its node, row and n_out are read in place and its
        rows get their world-frame normals in row_normal.  append: the cloud was run with append, so the rows an earlier call of this
        batch wrote (n_rows) stay as they are"""
        d = self.descriptor(params, depth, pose, n_images, frame_index, cloud, append)
        _run_normals(ctx, "prs_depth_normals_batch_run", C.byref(params), C.byref(d))
        if cloud is not None:
            self.n_rows.copy_(cloud.n_out)  # on the stream of the launch: the next append starts behind these rows
        return self.normal

    def rows_of(self, index):
        """row_normal gathered on the device by index [B, n] (any integer type), the input row of every output row as
        ops.WorldVoxelBatch keeps it in `index`: [B, n, 4] float32.  An index outside [0, row_stride) gives a row of zeros"""
        import torch
        if self.row_normal is None:
            raise ValueError("this batch was built without row_stride: it has no rows")
        if index.dim() != 2 or int(index.shape[0]) != self.batch or index.dtype.is_floating_point:
            raise ValueError("index must be an integer tensor [%d, n]" % self.batch)
        i = index.to(torch.int64)
        inside = (i >= 0) & (i < self.row_stride)
        rows = torch.gather(self.row_normal, 1, i.clamp(0, self.row_stride - 1).unsqueeze(-1).expand(-1, -1, 4))
        return torch.where(inside.unsqueeze(-1), rows, torch.zeros((), dtype=rows.dtype, device=rows.device))


# ---- TSDF fusion: depth images to a truncated signed distance volume and its surface (include/proslam_hip_tsdf.h) ----
def tsdf_params(camera, voxel_size=configs.TSDF["voxel_size"], truncation=configs.TSDF["truncation"],
                max_weight=configs.TSDF["max_weight"], min_weight=configs.TSDF["min_weight"], range_min=configs.TSDF["range_min"],
                range_max=configs.TSDF["range_max"], depth_type="u16", scale=1.0, sensor_in_robot=None):
    """prs_tsdf_params.  camera: a dictionary with fx, fy, cx, cy (configs.*["camera"]); voxel_size and truncation in metres; a
    voxel's weight saturates at max_weight (>= 1); the surface call reads the voxels whose weight is at least min_weight;
    range_min / range_max, depth_type, scale and sensor_in_robot as in depth_cloud_params.  Raises ValueError on every value the
    library refuses"""
    p = _lib_tsdf.TsdfParams()
    p.depth_type = _depth_type(depth_type, known=True)
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.voxel_size, p.truncation = float(np.float32(voxel_size)), float(np.float32(truncation))
        p.max_weight, p.min_weight = float(np.float32(max_weight)), float(np.float32(min_weight))
    p.depth_scaling_factor_to_meters = float(scale)
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    p.range_min, p.range_max = float(range_min), float(range_max)
    S = np.eye(4, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(4, 4)
    p.sensor_in_robot[:] = [float(x) for x in S.reshape(16)]
    values = [p.depth_scaling_factor_to_meters, p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max, p.voxel_size, p.truncation,
              p.max_weight, p.min_weight] + list(p.sensor_in_robot)
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not p.depth_scaling_factor_to_meters > 0.0:
        raise ValueError("scale must be positive as a float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    if not (p.voxel_size > 0.0 and p.truncation > 0.0):
        raise ValueError("voxel_size and truncation must be positive as float32")
    if not p.max_weight >= 1.0:
        raise ValueError("max_weight must be at least 1")
    return p


class TsdfVolumeBatch:
    """the TSDF volumes of B sequences, nx x ny x nz voxels each, fed with up to `frames` depth images of rows x cols pixels a call:
    owns volume [B, nz, ny, nx, 2] (tsdf, weight), origin [B, 4] (the world position of the corner of voxel (0, 0, 0); set it before
    the first call), n_updates [B, frames], n_skipped [B] and status [B] of the integrate call and, with out_stride, xyz and normal
    [B, out_stride, 4], cell [B, out_stride], n_out, n_total and surface_status [B] of the surface call, and both workspaces."""

    def __init__(self, batch, nx, ny, nz, frames, rows, cols, out_stride=None, device=0):
        import torch
        B, F = int(batch), int(frames)
        if B < 1 or F < 1 or int(rows) < 1 or int(cols) < 1 or int(nx) < 1 or int(ny) < 1 or int(nz) < 1 or \
                (out_stride is not None and int(out_stride) < 1):
            raise ValueError("batch, nx, ny, nz, frames, rows, cols and out_stride must be at least 1")
        if int(nx) * int(ny) * int(nz) > 0x7fffffff // 3:
            raise ValueError("nx * ny * nz must stay within (2^31 - 1) / 3")
        lib = _lib_tsdf.load()
        self.batch, self.frames, self.rows, self.cols = B, F, int(rows), int(cols)
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.out_stride = None if out_stride is None else int(out_stride)
        z = _zeros_on(device)
        self.volume = z((B, self.nz, self.ny, self.nx, 2), torch.float32)
        self.origin = z((B, 4), torch.float32)
        self.n_updates, self.n_skipped, self.status = z((B, F), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        nbytes = int(lib.prs_tsdf_workspace_bytes(B, F))
        if nbytes < 1:
            raise ValueError("batch * frames must stay below 2^31")
        self.workspace = z((nbytes,), torch.uint8)
        n = self.out_stride
        self.xyz = z((B, n, 4), torch.float32) if n else None
        self.normal = z((B, n, 4), torch.float32) if n else None
        self.cell = z((B, n), torch.int32) if n else None
        self.n_out, self.n_total, self.surface_status = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.surface_workspace = z((int(lib.prs_tsdf_surface_workspace_bytes(B, self.nx, self.ny, self.nz)),), torch.uint8)

    def clear(self):
        """every voxel back to never observed: a memset on torch's current stream (asynchronous)"""
        self.volume.zero_()

    def descriptor(self, params, depth, pose, n_images=None, frame_index=None):
        """the prs_tsdf_batch of device tensors: depth [B, frames, rows, cols (a view of longer rows is allowed: the pitch)] of
        params' depth type, pose [B, pose_stride, 16] float32, n_images [B] int32 or None = frames, frame_index [B, frames] int32 or
        None"""
        import torch
        B, F = self.batch, self.frames
        dtype = torch.uint16 if params.depth_type == DEPTH_U16 else torch.float32
        if depth.dtype != dtype or depth.dim() != 4 or tuple(depth.shape[:3]) != (B, F, self.rows) or int(depth.shape[3]) < self.cols or \
                depth.stride(3) != 1:
            raise ValueError("depth must be a %s tensor [%d, %d, %d, >= %d] with contiguous rows" % (dtype, B, F, self.rows, self.cols))
        if not _follow(depth, self.rows, strict=True):
            raise ValueError("the images of depth must follow one another at rows * pitch")
        if pose.dim() != 3 or int(pose.shape[0]) != B or int(pose.shape[2]) != 16 or pose.dtype != torch.float32 or not pose.is_contiguous():
            raise ValueError("pose must be a contiguous float32 [%d, pose_stride, 16]" % B)
        d = _lib_tsdf.TsdfBatch()
        d.batch, d.frames, d.rows, d.cols = B, F, self.rows, self.cols
        d.pitch, d.pose_stride = int(depth.stride(2)) * depth.element_size(), int(pose.shape[1])
        d.nx, d.ny, d.nz = self.nx, self.ny, self.nz
        d.depth, d.pose = depth.data_ptr(), pose.data_ptr()
        d.n_images = _n_images_ptr(n_images, B)
        d.frame_index = _int32_ptr(frame_index, "frame_index", (B, F))
        for name in ("origin", "volume", "n_updates", "n_skipped", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        return d

    def surface_descriptor(self, count_only=False):
        """the prs_tsdf_surface_batch of this batch's tensors"""
        if self.out_stride is None and not count_only:
            raise ValueError("this batch was built without out_stride: it has no rows for a surface")
        d = _lib_tsdf.TsdfSurfaceBatch()
        d.batch, d.nx, d.ny, d.nz, d.out_stride = self.batch, self.nx, self.ny, self.nz, self.out_stride or 0
        d.origin, d.volume = self.origin.data_ptr(), self.volume.data_ptr()
        d.n_out, d.n_total, d.status = self.n_out.data_ptr(), self.n_total.data_ptr(), self.surface_status.data_ptr()
        d.workspace = self.surface_workspace.data_ptr()
        if not count_only:
            d.xyz, d.normal, d.cell = self.xyz.data_ptr(), self.normal.data_ptr(), self.cell.data_ptr()
        return d

    def integrate(self, ctx, params, depth, pose, n_images=None, frame_index=None):
        """enqueue the fusion of every sequence's images into its volume (asynchronous) and return volume; per-sequence status lands
        in self.status.  Calls add up: a long sequence is fed `frames` images at a time"""
        d = self.descriptor(params, depth, pose, n_images, frame_index)
        _run_tsdf(ctx, "prs_tsdf_integrate_batch_run", C.byref(params), C.byref(d))
        return self.volume

    def surface(self, ctx, params):
        """enqueue the surface of every volume (asynchronous) -> (xyz, normal, n_out): the first n_out[b] rows of xyz[b] and
        normal[b] are the zero crossings and their normals, which formats.write_ply(path, xyz[b, :n], normals=normal[b, :n]) takes as
        they are; PRS_ERR_CAPACITY lands in self.surface_status[b] when out_stride rows did not hold them all (n_total[b])"""
        d = self.surface_descriptor()
        _run_tsdf(ctx, "prs_tsdf_surface_batch_run", C.byref(params), C.byref(d))
        return self.xyz, self.normal, self.n_out

    def count(self, ctx, params):
        """enqueue the count-only surface call (asynchronous): n_total and surface_status; n_out becomes 0"""
        d = self.surface_descriptor(count_only=True)
        _run_tsdf(ctx, "prs_tsdf_surface_batch_run", C.byref(params), C.byref(d))
        return self.n_total


# ---- TSDF raycast: a fused volume rendered into depth and normal images (include/proslam_hip_tsdf_raycast.h) ----
TSDF_RAYCAST_MAX_STEPS = 1048576.0                   # steps the diagonal of a volume may hold


def tsdf_raycast_params(camera, voxel_size=configs.TSDF["voxel_size"], step=configs.TSDF_RAYCAST["step"],
                        min_weight=configs.TSDF_RAYCAST["min_weight"], range_min=configs.TSDF_RAYCAST["range_min"],
                        range_max=configs.TSDF_RAYCAST["range_max"], sensor_in_robot=None):
    """prs_tsdf_raycast_params.  camera: a dictionary with fx, fy, cx, cy of the rendered images; voxel_size: the volume's, in
    metres; step: metres of z depth between two samples of a ray; a voxel whose weight is below min_weight counts as unobserved;
    range_min / range_max bound the z depth of a ray's samples and of its hit; sensor_in_robot as in tsdf_params.  Raises ValueError
    on every value the library refuses whatever the volume is"""
    p = _lib_tsdf_raycast.TsdfRaycastParams()
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.voxel_size, p.step, p.min_weight = float(np.float32(voxel_size)), float(np.float32(step)), float(np.float32(min_weight))
        p.range_min, p.range_max = float(np.float32(range_min)), float(np.float32(range_max))
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    S = np.eye(4, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(4, 4)
    p.sensor_in_robot[:] = [float(x) for x in S.reshape(16)]
    values = [p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max, p.voxel_size, p.step, p.min_weight] + list(p.sensor_in_robot)
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    if not (p.voxel_size > 0.0 and p.step > 0.0):
        raise ValueError("voxel_size and step must be positive as float32")
    return p


class TsdfRaycastBatch:
    """the images rendered out of the volumes of an ops.TsdfVolumeBatch, `views` images of rows x cols pixels per sequence: owns
    depth [B, views, rows, cols] float32 metres (0 = no surface), normal [B, views, rows, cols, 4] (the model's normal in the
    camera's frame and 1, or zeros), n_hit [B, views], n_skipped [B], status [B] and the workspace; reads volumes.volume and
    volumes.origin in place.  depth is a float32 depth image at scale 1: DepthCloudBatch, DepthNormalsBatch and
    TsdfVolumeBatch.integrate take it as it stands with params of depth_type "f32" and scale 1."""

    def __init__(self, ctx, volumes, views, rows, cols):
        import torch
        V = int(views)
        if V < 1 or int(rows) < 1 or int(cols) < 1:
            raise ValueError("views, rows and cols must be at least 1")
        if int(rows) * int(cols) > 0x7fffffff:
            raise ValueError("rows * cols must stay below 2^31")
        lib = _lib_tsdf_raycast.load()
        self.ctx, self.volumes = ctx, volumes
        B = self.batch = volumes.batch
        self.views, self.rows, self.cols = V, int(rows), int(cols)
        nbytes = int(lib.prs_tsdf_raycast_workspace_bytes(B, V))
        if nbytes < 1:
            raise ValueError("batch * views must stay below 2^31")
        z = _zeros_on(volumes.volume.device)
        self.depth = z((B, V, self.rows, self.cols), torch.float32)
        self.normal = z((B, V, self.rows, self.cols, 4), torch.float32)
        self.n_hit, self.n_skipped, self.status = z((B, V), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, pose, view_index=None, n_views=None):
        """the prs_tsdf_raycast_batch of device tensors: pose [B, pose_stride, 16] float32, view_index [B, views] int32 or None (view
        r takes pose r), n_views [B] int32 or None = views"""
        import torch
        B, V, vol = self.batch, self.views, self.volumes
        if pose.dim() != 3 or int(pose.shape[0]) != B or int(pose.shape[2]) != 16 or pose.dtype != torch.float32 or not pose.is_contiguous():
            raise ValueError("pose must be a contiguous float32 [%d, pose_stride, 16]" % B)
        d = _lib_tsdf_raycast.TsdfRaycastBatch()
        d.batch, d.views, d.rows, d.cols = B, V, self.rows, self.cols
        d.pitch, d.pose_stride = self.cols * 4, int(pose.shape[1])
        d.nx, d.ny, d.nz = vol.nx, vol.ny, vol.nz
        d.origin, d.volume, d.pose = vol.origin.data_ptr(), vol.volume.data_ptr(), pose.data_ptr()
        d.view_index = _int32_ptr(view_index, "view_index", (B, V))
        d.n_views = _int32_ptr(n_views, "n_views", (B,))
        for name in ("depth", "normal", "n_hit", "n_skipped", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        return d

    def run(self, params, pose, view_index=None, n_views=None):
        """enqueue the rendering of every sequence's views (asynchronous) -> (depth, normal, n_hit); per-sequence status lands in
        self.status.  Raises ValueError when the volume's diagonal holds more than 2^20 steps, which the library refuses"""
        vol = self.volumes
        f32 = np.float32
        with np.errstate(over="ignore"):
            steps = ((f32(vol.nx) + f32(vol.ny)) + f32(vol.nz)) * f32(params.voxel_size) / f32(params.step)
        if not steps <= f32(TSDF_RAYCAST_MAX_STEPS):
            raise ValueError("(nx + ny + nz) * voxel_size / step must stay within 2^20: the steps a ray may take")
        d = self.descriptor(pose, view_index, n_views)
        _run_tsdf_raycast(self.ctx, "prs_tsdf_raycast_batch_run", C.byref(params), C.byref(d))
        return self.depth, self.normal, self.n_hit


# ---- TSDF mesh: a fused volume as an indexed quad mesh, by surface nets (include/proslam_hip_tsdf_mesh.h) ----
TSDF_MESH_OUTPUTS = ("normal", "cube", "edge")


class TsdfMeshBatch:
    """the meshes of the volumes of an ops.TsdfVolumeBatch, up to vertex_stride vertices and quad_stride quads per sequence: owns
    vertex [B, vertex_stride, 4] (x, y, z and the crossings it averages), quad [B, quad_stride, 4] int32 (vertex rows of the
    sequence, counter-clockwise seen from the observed free side), n_vertices, n_vertices_total, n_quads, n_quads_total and status
    [B], the workspace and, as `outputs` names them, normal [B, vertex_stride, 4], cube [B, vertex_stride] and edge [B, quad_stride]
    (the voxel of a vertex's cube; the surface call's `cell` of a quad's crossing); reads volumes.volume and volumes.origin in
    place."""

    def __init__(self, volumes, vertex_stride, quad_stride, outputs=TSDF_MESH_OUTPUTS):
        import torch
        nv, nq = int(vertex_stride), int(quad_stride)
        if nv < 1 or nq < 1:
            raise ValueError("vertex_stride and quad_stride must be at least 1")
        outputs = tuple(outputs)
        if any(name not in TSDF_MESH_OUTPUTS for name in outputs):
            raise ValueError("outputs: any of %s" % ", ".join(TSDF_MESH_OUTPUTS))
        lib = _lib_tsdf_mesh.load()
        self.volumes, self.vertex_stride, self.quad_stride = volumes, nv, nq
        B = self.batch = volumes.batch
        nbytes = int(lib.prs_tsdf_mesh_workspace_bytes(B, volumes.nx, volumes.ny, volumes.nz))
        if nbytes < 1:
            raise ValueError("nx * ny * nz must stay within (2^31 - 1) / 3 and batch * ceil(nx * ny * nz / 1024) within 2^24 - 1")
        z = _zeros_on(volumes.volume.device)
        self.vertex, self.quad = z((B, nv, 4), torch.float32), z((B, nq, 4), torch.int32)
        self.normal = z((B, nv, 4), torch.float32) if "normal" in outputs else None
        self.cube = z((B, nv), torch.int32) if "cube" in outputs else None
        self.edge = z((B, nq), torch.int32) if "edge" in outputs else None
        self.n_vertices, self.n_vertices_total = z((B,), torch.int32), z((B,), torch.int32)
        self.n_quads, self.n_quads_total, self.status = z((B,), torch.int32), z((B,), torch.int32), z((B,), torch.int32)
        self.workspace = z((nbytes,), torch.uint8)

    def descriptor(self, count_only=False):
        """the prs_tsdf_mesh_batch of this batch's tensors and its volumes'"""
        vol = self.volumes
        d = _lib_tsdf_mesh.TsdfMeshBatch()
        d.batch, d.nx, d.ny, d.nz = self.batch, vol.nx, vol.ny, vol.nz
        d.vertex_stride, d.quad_stride = self.vertex_stride, self.quad_stride
        d.origin, d.volume = vol.origin.data_ptr(), vol.volume.data_ptr()
        for name in ("n_vertices", "n_vertices_total", "n_quads", "n_quads_total", "status", "workspace"):
            setattr(d, name, getattr(self, name).data_ptr())
        if not count_only:
            for name in ("vertex", "quad") + TSDF_MESH_OUTPUTS:
                t = getattr(self, name)
                setattr(d, name, None if t is None else t.data_ptr())
        return d

    @staticmethod
    def _checked(params):
        """raises ValueError on the params the library refuses: of prs_tsdf_params the call reads voxel_size and min_weight"""
        if not (np.isfinite(params.voxel_size) and params.voxel_size > 0.0 and np.isfinite(params.min_weight)):
            raise ValueError("voxel_size must be finite and positive, min_weight finite")

    def run(self, ctx, params):
        """enqueue the mesh of every volume (asynchronous) -> (vertex, quad, n_vertices, n_quads): the first n_vertices[b] rows of
        vertex[b] and the first n_quads[b] rows of quad[b]; PRS_ERR_CAPACITY lands in self.status[b] when a stride did not hold them
        all (n_vertices_total[b], n_quads_total[b])"""
        self._checked(params)
        d = self.descriptor()
        _run_tsdf_mesh(ctx, "prs_tsdf_mesh_batch_run", C.byref(params), C.byref(d))
        return self.vertex, self.quad, self.n_vertices, self.n_quads

    def count(self, ctx, params):
        """enqueue the count-only call (asynchronous) -> (n_vertices_total, n_quads_total); n_vertices and n_quads become 0"""
        self._checked(params)
        d = self.descriptor(count_only=True)
        _run_tsdf_mesh(ctx, "prs_tsdf_mesh_batch_run", C.byref(params), C.byref(d))
        return self.n_vertices_total, self.n_quads_total

    def mesh_of(self, b):
        """the mesh of sequence b after run (synchronises to read its two counts) -> (xyz [n, 4], normal [n, 4] or None,
        triangles [2 * n_quads, 3] int32) as device tensors: the triangles (v0, v1, v2) and (v0, v2, v3) of quad i are rows 2 i and
        2 i + 1, which formats.write_ply(path, xyz, normals=normal, faces=triangles) takes once they are on the host.  Raises
        ValueError when the sequence overflowed a stride: its quads may then name vertices that were not written"""
        b = int(b)
        if not 0 <= b < self.batch:
            raise ValueError("b must lie in [0, %d)" % self.batch)
        if int(self.status[b]) != 0:
            raise ValueError("sequence %d holds %d vertices and %d quads: more than vertex_stride or quad_stride"
                             % (b, int(self.n_vertices_total[b]), int(self.n_quads_total[b])))
        n, m = int(self.n_vertices[b]), int(self.n_quads[b])
        quad = self.quad[b, :m]
        triangles = quad[:, [0, 1, 2, 0, 2, 3]].reshape(2 * m, 3).contiguous()
        return self.vertex[b, :n], (None if self.normal is None else self.normal[b, :n]), triangles


# ---- dense align: a live depth image against a rendered model view, point-to-plane on SE(3) (include/proslam_hip_dense_align.h) ----
DENSE_ALIGN_RESULT_DTYPE = np.dtype([("H", np.float32, (6, 6)), ("b", np.float32, (6,)), ("chi_inliers", np.float32),
                                     ("chi_total", np.float32), ("num_inliers", np.int32), ("num_outliers", np.int32),
                                     ("num_rejected", np.int32), ("num_invalid", np.int32), ("num_unmatched", np.int32),
                                     ("num_samples", np.int32), ("status", np.int32), ("iterations", np.int32),
                                     ("steps_taken", np.int32), ("warnings", np.int32), ("reserved", np.int32, (2,))])


def dense_align_params(camera, depth_type="u16", scale=1.0, max_distance=configs.DENSE_ALIGN["max_distance"],
                       min_normal_cos=configs.DENSE_ALIGN["min_normal_cos"], robustifier=configs.DENSE_ALIGN["robustifier"],
                       chi_threshold=configs.DENSE_ALIGN["chi_threshold"], damping=configs.DENSE_ALIGN["damping"],
                       max_iterations=10, min_num_inliers=configs.DENSE_ALIGN["min_num_inliers"],
                       range_min=configs.DENSE_ALIGN["range_min"], range_max=configs.DENSE_ALIGN["range_max"], linearize_only=0):
    """prs_dense_align_params.  camera: a dictionary with fx, fy, cx, cy of both images; depth_type and scale: the live image's, as in
    depth_cloud_params; max_distance (metres) and min_normal_cos: the two gates; robustifier "clamp" / "saturated" or a
    PRS_ROBUSTIFIER_* value; chi_threshold in square metres of point-to-plane distance.  Raises ValueError on every value the library
    refuses"""
    p = _lib_dense_align.DenseAlignParams()
    p.depth_type = _depth_type(depth_type, known=True)
    if isinstance(robustifier, str):
        if robustifier not in ("clamp", "saturated"):
            raise ValueError('robustifier: "clamp" or "saturated"')
        p.robustifier = _lib.ROBUSTIFIER_SATURATED if robustifier == "saturated" else _lib.ROBUSTIFIER_CLAMP
    else:
        p.robustifier = int(robustifier)
    with np.errstate(over="ignore"):  # a value beyond float32 becomes inf and is refused below
        p.depth_scaling_factor_to_meters = float(np.float32(scale))
        p.max_distance, p.min_normal_cos = float(np.float32(max_distance)), float(np.float32(min_normal_cos))
        p.chi_threshold, p.damping = float(np.float32(chi_threshold)), float(np.float32(damping))
        p.range_min, p.range_max = float(np.float32(range_min)), float(np.float32(range_max))
    p.fx, p.fy, p.cx, p.cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
    p.max_iterations, p.min_num_inliers, p.linearize_only = int(max_iterations), int(min_num_inliers), int(linearize_only)
    values = [p.depth_scaling_factor_to_meters, p.fx, p.fy, p.cx, p.cy, p.range_min, p.range_max, p.max_distance, p.min_normal_cos,
              p.chi_threshold, p.damping]
    if not np.isfinite(values).all():
        raise ValueError("every parameter must be finite as a float32")
    if not p.depth_scaling_factor_to_meters > 0.0 or not p.max_distance > 0.0:
        raise ValueError("scale and max_distance must be positive as float32")
    if not 0.0 <= p.range_min <= p.range_max:
        raise ValueError("0 <= range_min <= range_max must hold")
    if p.chi_threshold < 0.0 or p.damping < 0.0 or not -1.0 <= p.min_normal_cos <= 1.0:
        raise ValueError("chi_threshold and damping must not be negative, min_normal_cos must lie in [-1, 1]")
    if p.robustifier not in (_lib.ROBUSTIFIER_CLAMP, _lib.ROBUSTIFIER_SATURATED):
        raise ValueError("robustifier: PRS_ROBUSTIFIER_CLAMP or PRS_ROBUSTIFIER_SATURATED")
    if p.max_iterations < 0 or (p.max_iterations < 1 and not p.linearize_only):
        raise ValueError("max_iterations must be at least 1 (0 with linearize_only)")
    return p


def _pair_images(t, name, dtype, batch, rows, cols, channels=None):
    """a tensor [B, rows, >= cols] (channels: [B, rows, cols, channels], contiguous) of one image a pair, or the same with a second
    dimension of length 1, as a raycast of one view and a depth batch of one frame have it -> (the tensor without it, pitch in bytes)"""
    if t.dim() == (4 if channels is None else 5) and int(t.shape[1]) == 1:
        t = t[:, 0]
    if channels is not None:
        if t.dtype != dtype or tuple(t.shape) != (batch, rows, cols, channels) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor [%d, %d, %d, %d]" % (name, dtype, batch, rows, cols, channels))
        return t, cols * channels * t.element_size()
    if t.dtype != dtype or t.dim() != 3 or tuple(t.shape[:2]) != (batch, rows) or int(t.shape[2]) < cols or t.stride(2) != 1 or \
            (batch > 1 and int(t.stride(0)) != rows * int(t.stride(1))):
        raise ValueError("%s must be a %s tensor [%d, %d, >= %d] with contiguous rows whose images follow one another at rows * pitch"
                         % (name, dtype, batch, rows, cols))
    return t, int(t.stride(1)) * t.element_size()


class DenseAlignBatch:
    """B independent pairs of a model view and a live image of rows x cols pixels: owns X [B, 16] (liveInModel, in / out: set it
    before run), result [B] (DENSE_ALIGN_RESULT_DTYPE through results()), mask (with mask=True; [B, N] of the last call through
    mask_of(step)) and the workspace, sized for step 1.  The model is the depth and normal of an ops.TsdfRaycastBatch of one view, the
    live image a depth batch of one frame and optionally the normal of an ops.DepthNormalsBatch, all read in place."""

    def __init__(self, ctx, batch, rows, cols, mask=False, device=0):
        import torch
        B = int(batch)
        if B < 1 or int(rows) < 1 or int(cols) < 1:
            raise ValueError("batch, rows and cols must be at least 1")
        lib = _lib_dense_align.load()
        self.ctx, self.batch, self.rows, self.cols = ctx, B, int(rows), int(cols)
        nbytes = int(lib.prs_dense_align_workspace_bytes(B, self.rows, self.cols, 1))
        if nbytes < 1:
            raise ValueError("rows * cols and batch * chunks must stay below 2^31")
        z = _zeros_on(device)
        self.X = z((B, 16), torch.float32)
        self.X[:, 0::5] = 1.0
        self.result = z((B, DENSE_ALIGN_RESULT_DTYPE.itemsize), torch.uint8)
        self.mask = z((B * self.rows * self.cols,), torch.uint8) if mask else None
        self.workspace = z((nbytes,), torch.uint8)

    def samples(self, step):
        """N of a call with this step"""
        return ((self.rows + step - 1) // step) * ((self.cols + step - 1) // step)

    def mask_of(self, step):
        """the [B, N] view of mask a call with this step wrote"""
        return self.mask[:self.batch * self.samples(step)].view(self.batch, -1)

    def descriptor(self, params, model_depth, model_normal, live_depth, live_normal=None, step=1):
        """the prs_dense_align_batch of device tensors: model_depth [B, rows, >= cols] float32 and model_normal [B, rows, cols, 4]
        float32 (or with a second dimension of 1 view), live_depth likewise of params' depth type, live_normal [B, rows, cols, 4] or
        None (no normal gate)"""
        import torch
        B, rows, cols = self.batch, self.rows, self.cols
        if int(step) < 1:
            raise ValueError("step must be at least 1")
        dtype = torch.uint16 if params.depth_type == DEPTH_U16 else torch.float32
        d = _lib_dense_align.DenseAlignBatch()
        d.batch, d.rows, d.cols, d.step = B, rows, cols, int(step)
        md, d.model_pitch = _pair_images(model_depth, "model_depth", torch.float32, B, rows, cols)
        ld, d.live_pitch = _pair_images(live_depth, "live_depth", dtype, B, rows, cols)
        mn, _ = _pair_images(model_normal, "model_normal", torch.float32, B, rows, cols, 4)
        d.model_depth, d.model_normal, d.live_depth = md.data_ptr(), mn.data_ptr(), ld.data_ptr()
        if live_normal is not None:
            d.live_normal = _pair_images(live_normal, "live_normal", torch.float32, B, rows, cols, 4)[0].data_ptr()
        d.X, d.result, d.workspace = self.X.data_ptr(), self.result.data_ptr(), self.workspace.data_ptr()
        d.mask = self.mask.data_ptr() if self.mask is not None else None
        return d

    def run(self, params, model_depth, model_normal, live_depth, live_normal=None, step=1):
        """enqueue one call (asynchronous): params.max_iterations times (linearise, step) on every step-th pixel -> X"""
        d = self.descriptor(params, model_depth, model_normal, live_depth, live_normal, step)
        _run_dense_align(self.ctx, "prs_dense_align_batch_run", C.byref(params), C.byref(d))
        return self.X

    def align(self, params, model_depth, model_normal, live_depth, live_normal=None, schedule=None):
        """enqueue the coarse-to-fine schedule, a list of (step, max_iterations) (None: configs.DENSE_ALIGN["schedule"]), on the same
        X -> X; result and mask are the last call's"""
        for step, iterations in (configs.DENSE_ALIGN["schedule"] if schedule is None else schedule):
            p = _lib_dense_align.DenseAlignParams.from_buffer_copy(bytes(params))
            p.max_iterations = int(iterations)
            self.run(p, model_depth, model_normal, live_depth, live_normal, step)
        return self.X

    def results(self):
        """result on the host (synchronises): a numpy array [B] of DENSE_ALIGN_RESULT_DTYPE"""
        return np.frombuffer(self.result.cpu().numpy().tobytes(), DENSE_ALIGN_RESULT_DTYPE)


class DenseTrackerBatch:
    """raycast -> align -> integrate for B sequences of depth images: a dense tracker over an ops.TsdfVolumeBatch built with
    frames = 1.  The poses are the camera's own (sensor_in_robot is the identity: a sensor offset is not handled here).  Owns pose
    [B, pose_stride, 16], the raycast of one view, the aligner and the live frame.  start() fuses frame 0 at pose 0 (set pose[:, 0]
    first); step(k, depth) renders the model at pose k - 1, aligns frame k from X = identity, writes pose k = pose k - 1 * X and fuses
    frame k there.  Every call is asynchronous and a whole step can be captured into a graph; k is written into the captured fills
    and copies, so a captured step is step k alone: replay it on another frame k (the tensor `depth` is read in place), not on another
    k."""

    def __init__(self, ctx, volumes, pose_stride, camera, depth_type="u16", scale=1.0, tsdf=None, raycast=None, align=None,
                 schedule=None, mask=False):
        import torch
        if volumes.frames != 1:
            raise ValueError("the volumes must be built with frames = 1: a step fuses one image")
        self.ctx, self.volumes, self.schedule = ctx, volumes, schedule
        B, rows, cols = volumes.batch, volumes.rows, volumes.cols
        self.batch, self.pose_stride = B, int(pose_stride)
        self.tsdf_params = tsdf_params(camera, depth_type=depth_type, scale=scale, **(tsdf or {}))
        self.raycast_params = tsdf_raycast_params(camera, voxel_size=self.tsdf_params.voxel_size, **(raycast or {}))
        self.align_params = dense_align_params(camera, depth_type=depth_type, scale=scale, **(align or {}))
        dev = volumes.volume.device
        z = _zeros_on(dev)
        self.pose = z((B, self.pose_stride, 16), torch.float32)
        self.pose[:, :, 0::5] = 1.0
        self.model = TsdfRaycastBatch(ctx, volumes, 1, rows, cols)
        self.aligner = DenseAlignBatch(ctx, B, rows, cols, mask=mask, device=dev)
        self.live = z((B, 1, rows, cols), torch.uint16 if self.tsdf_params.depth_type == DEPTH_U16 else torch.float32)
        self.index = z((B, 1), torch.int32)                       # the pose row of the view rendered and of the frame fused
        self.identity = z((B, 16), torch.float32)
        self.identity[:, 0::5] = 1.0
        self._prev, self._inverse, self._next = z((B, 16), torch.float32), z((B, 16), torch.float32), z((B, 16), torch.float32)

    def _integrate(self, k):
        """self.live into the volumes at pose[:, k]"""
        self.index.fill_(int(k))
        self.volumes.integrate(self.ctx, self.tsdf_params, self.live, self.pose, frame_index=self.index)

    def start(self, depth):
        """fuse frame 0, depth [B, rows, cols], at pose[:, 0]"""
        self.live[:, 0].copy_(depth)
        self._integrate(0)

    def step(self, k, depth):
        """frame k >= 1, depth [B, rows, cols]: pose[:, k] from the model seen at pose[:, k - 1], then the frame into the volume -> X"""
        if not 1 <= int(k) < self.pose_stride:
            raise ValueError("k must lie in [1, pose_stride)")
        self.index.fill_(int(k) - 1)
        depth_m, normal_m, _ = self.model.run(self.raycast_params, self.pose, view_index=self.index)
        self.live[:, 0].copy_(depth)
        self.aligner.X.copy_(self.identity)
        X = self.aligner.align(self.align_params, depth_m, normal_m, self.live, None, self.schedule)
        # pose_compose_batch(P, X) is P * X^-1: once on the identity for X^-1, once more for pose k - 1 * X
        self._prev.copy_(self.pose[:, int(k) - 1])
        pose_compose_batch(self.ctx, self.identity, X, self._inverse)
        pose_compose_batch(self.ctx, self._prev, self._inverse, self._next)
        self.pose[:, int(k)].copy_(self._next)
        self._integrate(k)
        return X


# ---- image rectifier: undistort and stereo-rectify raw frames in front of the extractors (include/proslam_hip.h prs_rectify_*) ----
DISTORTION_RADTAN = 0                                # PRS_DISTORTION_*
PIXEL_U8, PIXEL_U16, PIXEL_F32 = 0, 1, 2             # PRS_PIXEL_*
RECTIFY_BILINEAR, RECTIFY_NEAREST = 0, 1             # PRS_RECTIFY_*
_PIXEL_TYPES = {"u8": PIXEL_U8, "u16": PIXEL_U16, "f32": PIXEL_F32}
_PIXEL_NP = {PIXEL_U8: np.uint8, PIXEL_U16: np.uint16, PIXEL_F32: np.float32}
_INTERPOLATIONS = {"bilinear": RECTIFY_BILINEAR, "nearest": RECTIFY_NEAREST}


def rectify_params(pixel_type="u8", interpolation=None, border=0):
    """prs_rectify_params.  pixel_type "u8" / "u16" / "f32", interpolation "bilinear" / "nearest" (None: bilinear for u8, nearest
    otherwise: depth is never interpolated), border = the value of a pixel without a source (an integer type's must lie in its range)"""
    if pixel_type not in _PIXEL_TYPES:
        raise ValueError("pixel_type: one of %s" % (sorted(_PIXEL_TYPES),))
    t = _PIXEL_TYPES[pixel_type]
    if interpolation is None:
        interpolation = "bilinear" if t == PIXEL_U8 else "nearest"
    if interpolation not in _INTERPOLATIONS:
        raise ValueError("interpolation: one of %s" % (sorted(_INTERPOLATIONS),))
    i = _INTERPOLATIONS[interpolation]
    if i == RECTIFY_BILINEAR and t != PIXEL_U8:
        raise ValueError("bilinear interpolation is for u8 pixels only")
    if t != PIXEL_F32 and not (np.isfinite(border) and 0 <= border <= (255 if t == PIXEL_U8 else 65535)):
        raise ValueError("border must lie in the range of the pixel type")
    return _lib.RectifyParams(t, i, float(border), 0)


class RectifyMap:
    """one camera's rectification map, held in float64: K_src [3, 3] and dist (k1, k2, p1, p2, k3) of the raw camera, R [3, 3] taking
    its coordinates to the rectified camera's, K_dst [3, 3] of the rectified camera.  struct() is the prs_rectify_map (float32)."""

    def __init__(self, K_src, dist, R, K_dst):
        self.K_src, self.dist, self.R, self.K_dst = K_src, dist, R, K_dst

    def struct(self):
        m = _lib.RectifyMap()
        m.model = DISTORTION_RADTAN
        m.src_fx, m.src_fy, m.src_cx, m.src_cy = self.K_src[0, 0], self.K_src[1, 1], self.K_src[0, 2], self.K_src[1, 2]
        m.k1, m.k2, m.p1, m.p2, m.k3 = self.dist
        m.R[:] = [float(x) for x in self.R.reshape(9)]
        m.dst_fx, m.dst_fy, m.dst_cx, m.dst_cy = self.K_dst[0, 0], self.K_dst[1, 1], self.K_dst[0, 2], self.K_dst[1, 2]
        return m


def _finite32(a):
    """finite, also as the float32 the kernel is handed"""
    with np.errstate(over="ignore"):
        return bool(np.all(np.isfinite(a)) and np.all(np.isfinite(a.astype(np.float32))))


def _camera_matrix(K, what):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("%s must be a 3 x 3 camera matrix" % what)
    if not _finite32(K):
        raise ValueError("%s is not finite" % what)
    if np.float32(K[0, 0]) == 0 or np.float32(K[1, 1]) == 0:
        raise ValueError("%s is singular: a focal length is 0" % what)
    return K.copy()


def rectify_map(K_src, dist, R=None, K_dst=None):
    """one RectifyMap from the raw camera's matrix K_src [3, 3] and distortion (k1, k2, p1, p2[, k3]), the rotation R [3, 3] from its
    coordinates to the rectified camera's (None: the identity, undistortion only) and the rectified camera's matrix K_dst (None:
    K_src).  ValueError for a wrong shape, a value that is not finite (also as a float32), a zero focal length or a singular R."""
    Ks = _camera_matrix(K_src, "K_src")
    Kd = Ks.copy() if K_dst is None else _camera_matrix(K_dst, "K_dst")
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    if d.size not in (4, 5):
        raise ValueError("dist holds (k1, k2, p1, p2) or (k1, k2, p1, p2, k3)")
    d = np.concatenate([d, np.zeros(5 - d.size)])
    Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    if Rm.shape != (3, 3):
        raise ValueError("R must be 3 x 3")
    if not (_finite32(d) and _finite32(Rm)):
        raise ValueError("dist or R is not finite")
    if abs(np.linalg.det(Rm)) < 1e-12:
        raise ValueError("R is singular")
    return RectifyMap(Ks, d, Rm.copy(), Kd)


def stereo_rectification(K_l, D_l, K_r, D_r, R_rl, t_rl, image_size=None):
    """(map_left, map_right, camera) of a calibrated stereo pair, on the host in float64.  BUILD-DEFINED (the reference is handed
    rectified images).  R_rl [3, 3], t_rl [3]: the pose of the right camera in the left camera's frame (X_l = R_rl X_r + t_rl).
    The rectified x axis runs along the baseline, e1 = t / |t|; e2 = (0, 0, 1) x e1 normalised keeps the left camera's viewing
    direction as far as that allows; e3 = e1 x e2.  R_l has the rows e1, e2, e3 and R_r = R_l R_rl: both rectified cameras look
    along e3 and the right one stands at (|t|, 0, 0), so rows agree and u_l - u_r = fx |t| / z.  Both get the same matrix: fx = fy =
    the mean of the four focal lengths, the principal point the mean of the two.  camera has the keys of configs.*["camera"]
    (cols, rows from image_size = (cols, rows), None when it is not given; baseline_m = |t|)."""
    ml, mr = rectify_map(K_l, D_l), rectify_map(K_r, D_r)
    R_rl = np.asarray(R_rl, dtype=np.float64)
    t = np.asarray(t_rl, dtype=np.float64).reshape(-1)
    if R_rl.shape != (3, 3) or t.shape != (3,) or not (np.all(np.isfinite(R_rl)) and np.all(np.isfinite(t))):
        raise ValueError("R_rl must be a finite 3 x 3 rotation and t_rl a finite 3-vector")
    b = float(np.linalg.norm(t))
    if not b > 0.0:
        raise ValueError("t_rl is zero: the cameras have no baseline")
    e1 = t / b
    e2 = np.cross([0.0, 0.0, 1.0], e1)
    n2 = float(np.linalg.norm(e2))
    if not n2 > 1e-9:
        raise ValueError("the baseline runs along the optical axis")
    e2 = e2 / n2
    e3 = np.cross(e1, e2)
    R_l = np.stack([e1, e2, e3])
    R_r = R_l @ R_rl
    f = (ml.K_src[0, 0] + ml.K_src[1, 1] + mr.K_src[0, 0] + mr.K_src[1, 1]) / 4.0
    cx, cy = (ml.K_src[0, 2] + mr.K_src[0, 2]) / 2.0, (ml.K_src[1, 2] + mr.K_src[1, 2]) / 2.0
    K = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    cols, rows = (None, None) if image_size is None else (int(image_size[0]), int(image_size[1]))
    camera = {"fx": float(f), "fy": float(f), "cx": float(cx), "cy": float(cy), "cols": cols, "rows": rows, "baseline_m": b}
    return rectify_map(ml.K_src, ml.dist, R_l, K), rectify_map(mr.K_src, mr.dist, R_r, K), camera


class RectifyBatch:
    """the rectifier of `batch` images of src_shape = (rows, cols) into dst_shape (None: the same): owns the device array of maps,
    dst, n_border and status.  run(src) enqueues on the context's stream and returns dst, a [batch, rows, cols] view whose rows are
    padded to a multiple of four elements (one store per lane); the extractors and the depth stage take it in place with its pitch.
    stereo=True: two maps (left, right) and an even batch laid out as the left block [0 : batch / 2] then the right block, so a
    workgroup's run of images shares one map; left / right are the two halves of dst."""

    def __init__(self, ctx, params, maps, batch, src_shape, dst_shape=None, stereo=False):
        import torch
        maps = [maps] if isinstance(maps, RectifyMap) else list(maps)
        B = int(batch)
        if B < 1 or not maps:
            raise ValueError("batch and the number of maps must be at least 1")
        if stereo and (len(maps) != 2 or B % 2):
            raise ValueError("a stereo batch has two maps and an even number of images")
        self.ctx, self.params, self.batch, self.n_maps = ctx, params, B, len(maps)
        self.src_shape = (int(src_shape[0]), int(src_shape[1]))
        self.dst_shape = self.src_shape if dst_shape is None else (int(dst_shape[0]), int(dst_shape[1]))
        if min(self.src_shape + self.dst_shape) < 1:
            raise ValueError("image sizes must be at least 1")
        self.np_dtype = _PIXEL_NP.get(params.pixel_type, np.uint8)  # an unknown type is the library's to refuse
        self.dtype = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.float32: torch.float32}[self.np_dtype]
        dev, z = torch.device("cuda", ctx.device), _zeros_on(ctx.device)
        arr = (_lib.RectifyMap * len(maps))(*[m.struct() for m in maps])
        host = np.frombuffer(arr, dtype=np.uint8).copy()
        self.maps = torch.from_numpy(host).to(dev)
        self._dst, self.dst, _ = _padded_rows(z, (B, self.dst_shape[0]), self.dst_shape[1], self.dtype)
        self.n_border, self.status = z((B,), torch.int32), z((B,), torch.int32)
        self.map_of = None
        if stereo:
            self.map_of = torch.cat([torch.zeros(B // 2, dtype=torch.int32), torch.ones(B // 2, dtype=torch.int32)]).to(dev)
        self.left, self.right = (self.dst[: B // 2], self.dst[B // 2:]) if stereo else (None, None)

    def descriptor(self, src, map_of=None):
        rows, cols = self.src_shape
        if src.dtype != self.dtype or tuple(src.shape) != (self.batch, rows, cols) or src.stride(2) != 1 or \
                (self.batch > 1 and src.stride(0) != rows * src.stride(1)):
            raise ValueError("src must be a %s tensor [%d, %d, %d] with dense images (stride(0) = rows * pitch)" % (self.dtype, self.batch, rows, cols))
        d = _lib.RectifyBatch()
        d.map_of = _int32_ptr(self.map_of if map_of is None else map_of, "map_of", (self.batch,))
        es = src.element_size()
        d.batch, d.src_rows, d.src_cols, d.src_pitch, d.src = self.batch, rows, cols, int(src.stride(1)) * es, src.data_ptr()
        d.dst_rows, d.dst_cols, d.dst_pitch, d.dst = self.dst_shape[0], self.dst_shape[1], int(self._dst.stride(1)) * es, self._dst.data_ptr()
        d.n_maps, d.maps = self.n_maps, self.maps.data_ptr()
        d.n_border, d.status = self.n_border.data_ptr(), self.status.data_ptr()
        return d

    def run(self, src, map_of=None):
        """enqueue the rectification of src [batch, rows, cols] (asynchronous; map_of: int32 [batch] or None = the stereo layout's,
        else map 0 for every image); returns dst.  Per-image status and border counts land in self.status and self.n_border."""
        d = self.descriptor(src, map_of)
        _run(self.ctx, "prs_rectify_batch_run", C.byref(self.params), C.byref(d))
        return self.dst

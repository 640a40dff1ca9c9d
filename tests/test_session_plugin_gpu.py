"""The local-map manager's C++ adapter (LocalMapManagerHIP, tests/cpp/test_session_plugin.cpp) on one planted sequence, compared
with the Python path's bytes (ops.SessionBatch, itself byte-equal to tests/session_ref.py in test_session_gpu.py)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import session_cases as sc
import session_ref as ref
from test_session_gpu import Rig, _small

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_plugin_adapter(hip_ctx):
    exe = os.path.join(ROOT, "tests", "cpp", "test_session_plugin")
    assert os.path.exists(exe), "build() did not produce the adapter test program"
    # 3 m a frame: viewpoint splits, one lost frame, then the graph of 3 nodes is full
    n, rng = 14, np.random.default_rng(21)
    X = np.array([np.linalg.inv((sc.translation([0, 0.2, 3.0]) if k == 1 else np.eye(4)) @ _small(rng)) for k in range(n)]).astype(F)
    status, warnings = np.ones(n, np.int32), np.full(n, 8, np.int32)
    status[6] = 0
    tmp = tempfile.mkdtemp()
    names = {k: os.path.join(tmp, "session_plugin_%s.bin" % k) for k in ("X", "status", "warnings", "out")}
    X.tofile(names["X"])
    status.tofile(names["status"])
    warnings.tofile(names["warnings"])
    out = subprocess.run([exe, str(n), names["X"], names["status"], names["warnings"], names["out"]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    # the Python path, frame by frame
    rig = Rig(1, n, 64, 3, 3)
    reasons, statuses, poses, predictions = [], [], [], []
    for k in range(n):
        rig.step(hip_ctx, 10, 0.25, X[k: k + 1], status[k: k + 1], warnings[k: k + 1], np.zeros(1, np.int32))
        d = rig.sess.result_of(0)
        reasons.append(d["reason"])
        statuses.append(d["status"])
        poses.append(d["pose"])
        predictions.append(d["prediction"])
    rig.assert_equal()
    assert reasons.count(ref.SPLIT_VIEWPOINT) >= 1 and ref.SPLIT_LOST in reasons and ref.ERR_CAPACITY in statuses
    g, s = rig.graphs, rig.sess
    nn, ne = int(g.n_nodes[0].item()), int(g.n_edges[0].item())
    src, dst, Z, omega = g.edges_of(0)
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in (
        np.array(reasons, np.int32), np.array(statuses, np.int32), np.array(poses, F), np.array(predictions, F), np.array([nn, ne], np.int32),
        g.X[0, :nn].cpu().numpy(), src, dst, Z, omega, s.frame_node[0].cpu().numpy(), s.frame_pose[0].cpu().numpy(),
        s.unroll(hip_ctx)[0].cpu().numpy()))
    with open(names["out"], "rb") as f:
        got = f.read()
    assert got == want

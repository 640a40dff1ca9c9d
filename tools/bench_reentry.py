#!/usr/bin/env python3
"""Map re-entry beside the launches it stands next to, on the kitti map shape (4096 landmarks a map, three quarters full):
   the archive step (prs_session_step_archive_batch) against the plain step (prs_session_step_batch), alternating in one run, on
   frames that do not split and on frames that do (the archive copy: 109 bytes a landmark read and written);
   the re-entry launch (prs_session_reenter_batch: one map restored per sequence) and the closure merge that follows it.
Every figure is the median over `--reps` launches timed with device events after `--warmup` launches; the state a launch consumes
(graph counters, archive counters, map size) is put back between the timed launches, outside the event pairs.  The descriptors
are built once and the entry points are called directly, so that an event pair brackets one C call.  At 13 us such an interval is
still the launch path; `graph` therefore times the two steps with the host out of the interval altogether: GRAPH_LAUNCHES no-split
launches of one entry captured back to back and replayed, the replay's time divided by their number.

    python tools/bench_reentry.py [--batches 1,256,4096] [--reps 100] [--history 0]
    python tools/bench_reentry.py --plain-only --root /path/to/another/checkout   # the same harness on that checkout's plain step
prints one JSON line.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY, FILL = 4096, 3072
GRAPH_LAUNCHES = 20
ROW_BYTES = 109  # coords 16, desc 32, state 16, covariance 36, n_opt 4, inlier 1, n_meas 4
HBM_PEAK = 8.0e12  # bytes per second, MI355X


def median_us(events):
    return float(np.median([a.elapsed_time(b) for a, b in events])) * 1e3


def spread(events):
    t = np.array([a.elapsed_time(b) for a, b in events]) * 1e3
    return [float(np.percentile(t, 10)), float(np.percentile(t, 90))]


class Bench:
    def __init__(self, ctx, ops, configs, B, history, plain_only):
        import torch
        self.torch, self.ctx, self.ops, self.B = torch, ctx, ops, B
        dev = torch.device("cuda", 0)
        mm, mf = (history, 8) if history else (0, 1)
        self.maps, self.frames = ops.MapBatch(0, B, CAPACITY, mm, mf, 1, 1), ops.AlignFrames(0, B, 1, 1)
        self.graphs = ops.PoseGraphBatch(0, B, 4, 4, envelope_blocks=8)
        self.queries = ops.PlaceQueries(0, B, CAPACITY, 1)
        self.sess = ops.SessionBatch(0, self.maps, self.frames, self.graphs, GRAPH_LAUNCHES + 4, handover=self.queries)
        self.sp = ops.session_params(configs.get("kitti")["split"])
        g = torch.Generator(device="cuda").manual_seed(5)
        self.maps.coords.copy_(torch.rand(self.maps.coords.shape, device=dev, generator=g) * 20)
        self.maps.desc.copy_(torch.randint(0, 256, self.maps.desc.shape, device=dev, generator=g, dtype=torch.uint8))
        self.eye = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
        self.far = self.eye.clone()
        self.far[:, 11] = -11.0
        self.frames.result.view(torch.int32)[:, ops.AlignResult.status.offset // 4] = 1
        if plain_only:
            return
        K = 1
        pairs = types.SimpleNamespace(corr_stride=CAPACITY, result=torch.zeros((B * K, 52), dtype=torch.int32, device=dev),
                                      X=self.eye.clone(), corr=torch.zeros((B * K, CAPACITY, 3), dtype=torch.int32, device=dev),
                                      n_corr=torch.zeros((B * K,), dtype=torch.int32, device=dev))
        bank = types.SimpleNamespace(map_stride=2, node_of_map=torch.zeros((B, 2), dtype=torch.int32, device=dev))
        links = types.SimpleNamespace(candidates_flat=(torch.arange(B, dtype=torch.int32, device=dev) * 2).reshape(B, 1).contiguous())
        self.det = types.SimpleNamespace(batch=B, max_candidates=K, queries=self.queries, closures=types.SimpleNamespace(pairs=pairs),
                                         links=links, bank=bank)
        self.arch = ops.MapArchive(0, self.maps, 4, 2, with_history=bool(history))
        self.rb = ops.ReentryBatch(self.sess, self.maps, self.det, self.arch)
        from srrg2_proslam_amd import _lib
        r = _lib.PointAlignResult
        pairs.result[:, r.accepted.offset // 4], pairs.result[:, r.status.offset // 4] = 1, 1
        pairs.result[:, r.num_inliers.offset // 4], pairs.result[:, r.num_correspondences.offset // 4] = 2000, 2048
        idx = torch.arange(2048, dtype=torch.int32, device=dev)
        pairs.corr[:, :2048, 0], pairs.corr[:, :2048, 1] = idx, idx
        pairs.n_corr.fill_(2048)
        self.rp = ops.reentry_params(configs.REENTRY["kitti"], max_translation=1000.0)
        self.cp = ops.closure_merger_params(configs.get("kitti")["closure_merger"], configs.get("kitti")["camera"])

    def before_frame(self, split):
        """frame 1 of a fresh session over a map of FILL landmarks: no graph growth is carried from launch to launch"""
        s, g, m = self.sess, self.graphs, self.maps
        for t in (s.pose, s.prev, s.prediction):
            t.copy_(self.eye)
        s.slot.fill_(1)
        s.n_frames.fill_(1)
        s.cur_node.zero_()
        g.n_nodes.fill_(1)
        g.n_edges.zero_()
        m.n_points.fill_(FILL)
        self.frames.X.copy_(self.far if split else self.eye)
        if hasattr(self, "arch"):
            self.arch.n_slots.zero_()
            self.arch.slot_of_node.fill_(-1)

    def step_launches(self):
        """[(name, launch)]: the two entry points over descriptors built once"""
        import ctypes as C
        from srrg2_proslam_amd import _lib
        lib, h, sp = _lib.load(), self.ctx._h, C.byref(self.sp)
        self._keep = [self.sess.descriptor(), self.maps.descriptor()]
        sd, md = (C.byref(d) for d in self._keep)
        launches = [("plain", lambda: lib.prs_session_step_batch(h, sp, sd))]
        if hasattr(self, "rb"):
            self._keep.append(self.arch.descriptor())
            ad = C.byref(self._keep[2])
            launches.append(("archive", lambda: lib.prs_session_step_archive_batch(h, sp, sd, md, ad)))
        return launches

    def time_steps_graph(self, reps, warmup):
        """no-split frames, GRAPH_LAUNCHES launches of one entry per captured graph: microseconds per launch, host excluded"""
        torch = self.torch
        graphs = []
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.ctx.use_torch_stream()
            for name, launch in self.step_launches():
                self.before_frame(False)
                assert launch() == 0  # warm-up on the capture stream
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    for _ in range(GRAPH_LAUNCHES):
                        launch()
                graphs.append((name, g))
        torch.cuda.current_stream().wait_stream(s)
        self.ctx.use_torch_stream()
        torch.cuda.synchronize()
        events = {name: [] for name, _ in graphs}
        for i in range(warmup + reps):
            for name, g in graphs:
                self.before_frame(False)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                if i >= warmup:
                    events[name].append((a, b))
        torch.cuda.synchronize()
        assert int(self.sess.n_frames[0].item()) == 1 + GRAPH_LAUNCHES and not self.sess.status.any().item() and not self.sess.reason.any().item()
        return {name: dict(us=median_us(ev) / GRAPH_LAUNCHES, p10_p90=[v / GRAPH_LAUNCHES for v in spread(ev)]) for name, ev in events.items()}

    def time_steps(self, split, reps, warmup):
        torch = self.torch
        launches = self.step_launches()
        events = {name: [] for name, _ in launches}
        for i in range(warmup + reps):
            for name, launch in launches:
                self.before_frame(split)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                if i >= warmup:
                    events[name].append((a, b))
        torch.cuda.synchronize()
        assert int(self.sess.reason[0].item()) == (1 if split else 0) and not self.sess.status.any().item()
        return {name: dict(us=median_us(ev), p10_p90=spread(ev)) for name, ev in events.items()}

    def time_reentry(self, reps, warmup):
        torch, ops = self.torch, self.ops
        # two splits leave m = 2, f = 1 and map 0 archived; the hand-over slot holds the finished map
        self.sess.reset()
        self.arch.clear()
        self.frames.X.copy_(self.eye)
        self.sess.step(self.ctx, self.sp)
        for _ in range(2):
            self.maps.n_points.fill_(FILL)
            self.frames.X.copy_(self.far)
            self.rb.step(self.ctx, self.sp)
        self.queries.xyz.copy_(self.arch.coords[:, 0])  # the finished map lies on the archived one: every correspondence merges
        self.queries.n_query.fill_(FILL)
        saved = [t.clone() for t in (self.sess.pose, self.sess.prev, self.sess.prediction)]
        ev_r, ev_m = [], []
        for i in range(warmup + reps):
            for t, v in zip((self.sess.pose, self.sess.prev, self.sess.prediction), saved):
                t.copy_(v)
            self.sess.cur_node.fill_(2)
            self.graphs.n_nodes.fill_(3)
            self.graphs.n_edges.fill_(2)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            self.rb.reenter(self.ctx, self.rp)
            e[1].record()
            ops.closure_merge_batch(self.ctx, self.cp, self.rb.merge_view)
            e[2].record()
            if i >= warmup:
                ev_r.append((e[0], e[1]))
                ev_m.append((e[1], e[2]))
        torch.cuda.synchronize()
        assert self.rb.reentered.all().item() and not self.rb.status.any().item() and int(self.sess.cur_node[0].item()) == 0
        merged = self.rb.merge_view.result[0].cpu().numpy().tolist()
        return dict(reenter_us=median_us(ev_r), reenter_p10_p90=spread(ev_r), closure_merge_us=median_us(ev_m), merge_result=merged)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--history", type=int, default=0, help="measurement history slots per landmark kept in the map and the archive")
    ap.add_argument("--plain-only", action="store_true", help="time prs_session_step_batch alone (works on a checkout without re-entry)")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from srrg2_proslam_amd import configs, ops
    ctx = ops.Context(0)
    ctx.use_torch_stream()
    out = dict(tool="bench_reentry", root=os.path.abspath(args.root), capacity=CAPACITY, fill=FILL, history=args.history, reps=args.reps, batches={})
    for B in [int(b) for b in args.batches.split(",")]:
        bench = Bench(ctx, ops, configs, B, args.history, args.plain_only)
        row = dict(no_split=bench.time_steps(False, args.reps, args.warmup), split=bench.time_steps(True, args.reps, args.warmup),
                   graph=bench.time_steps_graph(args.reps, args.warmup))
        if not args.plain_only:
            row.update(bench.time_reentry(args.reps, args.warmup))
            moved = 2.0 * B * FILL * (ROW_BYTES + 28 * args.history) + (2.0 * B * 8 * 96 if args.history else 0.0)
            extra = (row["split"]["archive"]["us"] - row["split"]["plain"]["us"]) * 1e-6
            row["archive_copy_bytes"] = moved
            row["archive_copy_bytes_per_s"] = moved / extra if extra > 0 else None
            row["reenter_bytes_per_s"] = moved / (row["reenter_us"] * 1e-6)
            row["hbm_peak_bytes_per_s"] = HBM_PEAK
        out["batches"][str(B)] = row
        del bench
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

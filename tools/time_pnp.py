"""PnPsolver on the device (afv_frame_pnp_hypotheses: three launches, every EPnP RANSAC hypothesis of every candidate of a relocalisation
and the Refine of every record) next to the same algorithm as a scalar host program (tools/pnp_host.cpp, g++ -O3 -ffp-contract=off,
compiled here).  One current frame of 1000 features, 10 candidates of 60 correspondences each, 35 hypotheses (what SetRansacParameters
asks for at Tracking's constants), on two workloads: every candidate false (each solver runs all its iterations inside its first
iterate(5): quirk Q1), and the same with one true candidate, whose refinement answers in its first round.

Host-to-host medians of --calls calls with [fastest, slowest], in one run:
  PnPsolver.batch through the Python wrapper (records and rows built inside the clock)
  afv_frame_pnp_hypotheses alone, records and rows built beforehand (what a C++ caller pays)
  the round-robin iterate(5) loop over the solvers (host scan, Python)
  the host program over all hypotheses of every candidate
  the host program with every candidate stopped at the hypothesis at which the round-robin loop left its solver (what the reference
  computes, with one Refine per record; a candidate the loop never reached pays its constructor only)
and the device's answers are compared with the host program's, bit for bit, in the same run.

    python tools/time_pnp.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_pnp.py --calls 20
(k_pnp_gather, k_pnp_hypotheses, k_pnp_refine)"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32
NC, NF, NMATCH, NHYP, MIN_INLIERS, EPSILON, TH2 = 10, 1000, 60, 35, 10, 0.5, 5.991
W, H, CAM = 640, 480, (520.0, 515.0, 318.5, 242.25)


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def world(n_true, seed=1):
    """a frame of NF features that are exact projections of NF points; candidate c matches NMATCH of them: the first n_true candidates to
    the right points (a fifth displaced: outliers), the others to a permutation (every match false)"""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = CAM
    u, v, z = rs.uniform(20, W - 20, NF), rs.uniform(20, H - 20, NF), rs.uniform(4, 8, NF)
    pos = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1).astype(f32)   # the camera sits at the origin
    Xc = pos.astype(np.float64)
    x, y = (fx * Xc[:, 0] / Xc[:, 2] + cx).astype(f32), (fy * Xc[:, 1] / Xc[:, 2] + cy).astype(f32)
    rows = np.full((NC, NF), -1, np.int32)
    for c in range(NC):
        feats = rs.permutation(NF)[:NMATCH]
        rows[c, feats] = feats if c < n_true else feats[rs.permutation(NMATCH)]
        if c < n_true:
            wrong = feats[:NMATCH // 5]
            rows[c, wrong] = wrong[::-1]
    return dict(x=x, y=y, pos=pos, rows=rows)


def round_robin(solvers):
    """Relocalization's loop (Tracking.cc:1190-1216): iterate(5) over the candidates until one answers or all say bNoMore"""
    alive = [True] * len(solvers)
    while any(alive):
        for c, s in enumerate(solvers):
            if not alive[c]:
                continue
            T, no_more, vb, n = s.iterate(5)
            if no_more:
                alive[c] = False
            if T is not None:
                return c, n
    return -1, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_pnp.py measures on the GPU: none found")
    pnp = importlib.import_module("anyfeature-vslam_amd.pnp")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "pnp_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "pnp_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).pnp_host
    host.restype = None
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    words = (NF + 31) // 32
    keys = ("n", "min_inliers", "index", "count", "degenerate", "pose", "inliers", "refined", "refined_count", "refined_pose", "refined_inliers")
    for label, n_true in (("all candidates false", 0), ("one candidate true", 1)):
        Wd = world(n_true)
        points = afv.MapPoints(ctx, NF)
        points.set(np.arange(NF, dtype=np.int32), pos=Wd["pos"])
        frame = afv.Frame(ctx, max_x=W, max_y=H, cap=NF)
        kps = np.zeros(NF, afv.KP_DTYPE)
        kps["x"], kps["y"] = Wd["x"], Wd["y"]
        frame.set_features(kps, np.zeros((NF, 32), np.uint8))
        eye = np.eye(3, dtype=f32)
        frame.set_pose(eye, np.zeros(3, f32), np.zeros(3, f32), *CAM)
        sigma2 = ctx.size_sigma(kps)[1]
        seeds = [7 + c for c in range(NC)]

        def batch():
            return afv.PnPsolver.batch(frame, points, Wd["rows"], seed=7, nhyp=NHYP, minInliers=MIN_INLIERS, epsilon=EPSILON, th2=TH2)
        solvers = batch()
        t_batch, t_call, t_scan, t_host, t_host_stop = [], [], [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            batch()
            t_batch.append(time.perf_counter() - t0)
        jobs = pnp.pnp_jobs(seeds, MIN_INLIERS, EPSILON, TH2)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            out = pnp.hypotheses(frame, points, jobs, Wd["rows"], nhyp=NHYP)
            t_call.append(time.perf_counter() - t0)
        winner = None
        for _ in range(a.calls):
            for s in solvers:
                s.mnIterations, s.mnBestInliers, s.best = 0, 0, None
            t0 = time.perf_counter()
            winner = round_robin(solvers)
            t_scan.append(time.perf_counter() - t0)
        # the host program over the same inputs
        cam, useeds, flags = np.asarray(CAM, f32), np.array(seeds, np.uint64), np.ones(NF, np.uint8)
        h = dict(n=np.zeros(NC, np.int32), min_inliers=np.zeros(NC, np.int32), index=np.zeros((NC, NF), np.int32), count=np.zeros((NC, NHYP), np.int32),
                 degenerate=np.zeros((NC, NHYP), np.uint8), pose=np.zeros((NC, NHYP, 12), f32), inliers=np.zeros((NC, NHYP, words), np.uint32),
                 refined=np.zeros((NC, NHYP), np.uint8), refined_count=np.zeros((NC, NHYP), np.int32), refined_pose=np.zeros((NC, NHYP, 12), f32),
                 refined_inliers=np.zeros((NC, NHYP, words), np.uint32))
        g = {k: np.zeros_like(v) for k, v in h.items()}   # the stopped runs write elsewhere

        def run_host(dst, stops=None):
            host(C.c_int(NC), C.c_int(NF), C.c_int(NHYP), C.c_int(words), None if stops is None else p_(stops), p_(cam), p_(useeds), C.c_int(MIN_INLIERS), C.c_float(EPSILON), C.c_float(TH2),
                 p_(Wd["x"]), p_(Wd["y"]), p_(sigma2), p_(Wd["pos"]), p_(flags), p_(Wd["rows"]), *[p_(dst[k]) for k in keys])
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host(h)
            t_host.append(time.perf_counter() - t0)
        same = all(h[k].tobytes() == np.ascontiguousarray(out[k]).tobytes() for k in keys)
        # what the reference runs: every candidate up to the hypothesis at which the round-robin loop left its solver
        stops = np.array([s.mnIterations for s in solvers], np.int32)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host(g, stops)
            t_host_stop.append(time.perf_counter() - t0)
        same_stopped = all(g[k][c][:stops[c]].tobytes() == h[k][c][:stops[c]].tobytes() for k in keys[3:] for c in range(NC))
        extra = dict(workload=label, candidates=NC, correspondences=float(np.mean(out["n"])), hypotheses=NHYP)
        stats("device: PnPsolver.batch through the Python wrapper", t_batch, **extra)
        stats("device: afv_frame_pnp_hypotheses alone, records built beforehand", t_call, equal_to_host_program=same, **extra)
        stats("host scan: the round-robin iterate(5) loop over the solvers (Python)", t_scan, winner=winner[0], inliers=winner[1],
              iterations_per_solver=[int(v) for v in stops], **extra)
        stats("host program: all %d hypotheses of every candidate" % NHYP, t_host, **extra)
        stats("host program: every candidate stopped where the round-robin loop left it (%d hypotheses in all)" % int(stops.sum()), t_host_stop,
              equal_to_the_full_run=same_stopped, **extra)
        frame.close()
        points.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

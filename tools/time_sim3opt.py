"""OptimizeSim3 on the device (afv_table_optimize_sim3: two launches, one wavefront per candidate) next to the same algorithm as a scalar
host program (tools/sim3opt_host.cpp, g++ -O3 -ffp-contract=off, compiled here).  One current keyframe of 1000 features, candidates of
150 correspondences (20 % outliers, 0.5 px of noise, a start a few per cent off); two workloads: 1 candidate and 10 candidates.
Host-to-host times over --calls calls each, median with [fastest, slowest], one JSON line per figure:

  OptimizeSim3Batch through the Python wrapper (records and rows built inside the clock)
  afv_table_optimize_sim3 alone, records and rows built beforehand (what a C++ caller pays)
  the host program over the same inputs

The device's answers are compared with the host program's, bit for bit, once per workload.

    python tools/time_sim3opt.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_sim3opt.py --calls 20
(k_sim3opt_gather, k_sim3opt_solve)"""
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
N1, NMATCH, CAP = 1000, 150, 1024
FX, FY, CX, CY = f32(517.3), f32(516.5), f32(318.6), f32(255.3)


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def rot(rs, amax):
    ax = rs.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rs.uniform(-amax, amax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def image(Xc):
    return (FX * (Xc[:, 0] / Xc[:, 2]) + CX).astype(f32), (FY * (Xc[:, 1] / Xc[:, 2]) + CY).astype(f32)


def world(nc, seed=1):
    """keyframe 0 with N1 features / points; candidate c matches NMATCH of them and sees map 2 = a planted Sim3 of map 1"""
    rs = np.random.RandomState(seed)
    cam = lambda R, t: dict(Rcw=R.astype(f32).reshape(9), tcw=t.astype(f32), fx=FX, fy=FY, cx=CX, cy=CY)
    R1, t1 = rot(rs, 0.3), rs.uniform(-1, 1, 3)
    X1 = np.stack([rs.uniform(-2, 2, N1), rs.uniform(-1.5, 1.5, N1), rs.uniform(3, 9, N1)], 1)
    pos = [(X1 - t1) @ R1]
    cams = {0: cam(R1, t1)}
    inf = (f32(1.0) / f32(1.2) ** (2 * rs.randint(0, 8, (nc + 1, N1)))).astype(f32)
    x, y = np.zeros((nc + 1, N1), f32), np.zeros((nc + 1, N1), f32)
    x[0], y[0] = image(X1)
    mp1 = np.arange(N1, dtype=np.int32)
    mp2, idx2 = np.full((nc, N1), -1, np.int32), np.full((nc, N1), -1, np.int32)
    starts = []
    for c in range(nc):
        R2, t2 = rot(rs, 0.3), rs.uniform(-1, 1, 3)
        R12, t12, s = rot(rs, 0.5), rs.uniform(-0.5, 0.5, 3), rs.uniform(0.5, 2.0)
        feat = np.sort(rs.permutation(N1)[:NMATCH])
        Xn = X1[feat].copy()
        Xn[:, :2] += rs.normal(0, 0.5, (NMATCH, 2)) * Xn[:, 2:3] / 517.0
        X2 = ((Xn - t12) @ R12) / s
        wrong = rs.permutation(NMATCH)[:NMATCH // 5]
        X2[wrong] = np.stack([rs.uniform(-2, 2, len(wrong)), rs.uniform(-1.5, 1.5, len(wrong)), rs.uniform(3, 9, len(wrong)) / s], 1)
        mp2[c, feat] = N1 + c * NMATCH + np.arange(NMATCH)
        k2 = rs.permutation(N1)[:NMATCH]
        idx2[c, feat] = k2
        x[c + 1], y[c + 1] = rs.uniform(0, 640, N1), rs.uniform(0, 480, N1)
        x[c + 1, k2], y[c + 1, k2] = image(X2)
        pos.append((X2 - t2) @ R2)
        cams[c + 1] = cam(R2, t2)
        starts.append((rot(rs, 0.02) @ R12, t12 + rs.uniform(-0.03, 0.03, 3), s * 1.03))
    return dict(cams=cams, pos=np.concatenate(pos).astype(f32), inf=inf, x=x, y=y, mp1=mp1, mp2=mp2, idx2=idx2, starts=starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_sim3opt.py measures on the GPU: none found")
    sim3 = importlib.import_module("anyfeature-vslam_amd.sim3")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "sim3opt_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "anyfeature-vslam_amd", "csrc"), "-shared", "-fPIC",
                    os.path.join(ROOT, "tools", "sim3opt_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).sim3opt_host
    host.restype = None
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    for nc in (1, 10):
        W = world(nc)
        table = afv.table.DescriptorTable(ctx, nc + 1, CAP)
        points = afv.MapPoints(ctx, len(W["pos"]))
        points.set(np.arange(len(W["pos"]), dtype=np.int32), pos=W["pos"])
        for s in range(nc + 1):
            table.set(s, np.zeros((N1, 32), np.uint8))
            table.set_geometry(s, W["x"][s], W["y"][s], np.ones(N1, f32))
            table.set_inf(s, W["inf"][s])
        cands = list(range(1, nc + 1))
        batch = lambda: afv.OptimizeSim3Batch(table, points, 0, cands, W["mp1"], W["mp2"], W["idx2"], W["cams"], W["starts"], th2=10, fix_scale=False)
        answers = batch()
        t_batch, t_call, t_host = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            batch()
            t_batch.append(time.perf_counter() - t0)
        jobs = sim3.sim3opt_jobs(W["cams"][0], [W["cams"][c] for c in cands], W["starts"], 10, False)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            res, state = sim3.optimize_sim3(table, points, [0] * nc, cands, jobs, W["mp1"], W["mp2"], W["idx2"])
            t_call.append(time.perf_counter() - t0)
        # the host program over the same inputs
        camrec, start = np.zeros((nc, 32), f32), np.zeros((nc, 13), f32)
        for c in range(nc):
            for o, cam in ((0, W["cams"][0]), (16, W["cams"][c + 1])):
                camrec[c, o:o + 9], camrec[c, o + 9:o + 12] = cam["Rcw"], cam["tcw"]
                camrec[c, o + 12:o + 16] = [cam["fx"], cam["fy"], cam["cx"], cam["cy"]]
            start[c, :9], start[c, 9:12], start[c, 12] = np.asarray(W["starts"][c][0], f32).reshape(9), W["starts"][c][1], W["starts"][c][2]
        th2, fix, flags = np.full(nc, 10, f32), np.zeros(nc, np.int32), np.ones(len(W["pos"]), np.uint8)
        x2, y2, inf2 = (np.ascontiguousarray(W[k][1:]) for k in ("x", "y", "inf"))
        x1, y1, inf1 = (np.ascontiguousarray(W[k][0]) for k in ("x", "y", "inf"))
        ints, doubles, hstate = np.zeros((nc, 9), np.int32), np.zeros((nc, 17), np.float64), np.zeros((nc, N1), np.uint8)

        def run_host():
            host(nc, N1, N1, p_(camrec), p_(start), p_(th2), p_(fix), p_(W["pos"]), p_(flags), p_(x1), p_(y1), p_(inf1), p_(W["mp1"]), p_(x2), p_(y2),
                 p_(inf2), p_(W["mp2"]), p_(W["idx2"]), p_(ints), p_(doubles), p_(hstate))
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host()
            t_host.append(time.perf_counter() - t0)
        same = True
        for c in range(nc):
            r = res[c]
            same &= [r.n_in, r.n_corr, r.n_bad, r.more_iterations, r.early, r.iterations[0], r.iterations[1], r.trials[0], r.trials[1]] == list(ints[c])
            same &= np.array(list(r.R12) + list(r.t12) + [r.s12] + list(r.chi2) + list(r.lam)).tobytes() == doubles[c].tobytes()
            same &= bool(np.array_equal(state[c, :N1], hstate[c]))
        extra = dict(candidates=nc, correspondences=float(np.mean([res[c].n_corr for c in range(nc)])),
                     inliers=float(np.mean([a_[0] for a_ in answers])), iterations=float(np.mean([sum(res[c].iterations) for c in range(nc)])),
                     trials=float(np.mean([sum(res[c].trials) for c in range(nc)])))
        stats("device: OptimizeSim3Batch through the Python wrapper", t_batch, **extra)
        stats("device: afv_table_optimize_sim3 alone, records built beforehand", t_call, equal_to_host_program=bool(same), **extra)
        stats("host program: tools/sim3opt_host.cpp", t_host, **extra)
        points.close()
        table.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

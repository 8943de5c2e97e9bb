"""Sim3Solver on the device (afv_table_sim3_hypotheses: two launches, every RANSAC hypothesis of every candidate of a loop check) next to
the same algorithm as a scalar host program (tools/sim3_host.cpp, g++ -O3 -ffp-contract=off, compiled here).  One current keyframe, 10
candidates of about 150 correspondences, 300 hypotheses each; two workloads: every candidate false (all 300 hypotheses are needed before
bNoMore), and one candidate true.  Host-to-host times over --calls calls each, median and spread, one JSON line per figure:

  Sim3Solver.batch through the Python wrapper (records and rows built inside the clock)
  afv_table_sim3_hypotheses alone, records and rows built beforehand (what a C++ caller pays)
  LoopClosing's round-robin iterate(5) loop over the returned solvers (host scan)
  the host program over the same inputs, all 300 hypotheses of every candidate
  the host program stopping each candidate where the reference's iterate would (what the reference actually runs)

The device's answers are compared with the host program's, bit for bit, in the same run.

    python tools/time_sim3.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_sim3.py --calls 20
(k_sim3_gather, k_sim3_hypotheses)"""
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
NC, N1, NMATCH, NHYP, CAP, MIN_INLIERS = 10, 1000, 150, 300, 1024, 20


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


def world(n_true, seed=1):
    """keyframe 0 with N1 features / points; candidate c matches NMATCH of them; the first n_true candidates see map 2 = a planted Sim3 of
    map 1 (20 % outliers, 0.5 px of noise), the others see unrelated points"""
    rs = np.random.RandomState(seed)
    cam = lambda R, t: dict(Rcw=R.astype(f32).reshape(9), tcw=t.astype(f32), fx=f32(517.3), fy=f32(516.5), cx=f32(318.6), cy=f32(255.3))
    R1, t1 = rot(rs, 0.3), rs.uniform(-1, 1, 3)
    X1 = np.stack([rs.uniform(-2, 2, N1), rs.uniform(-1.5, 1.5, N1), rs.uniform(3, 9, N1)], 1)
    pos = [(X1 - t1) @ R1]
    cams = {0: cam(R1, t1)}
    sigma2 = np.zeros((NC + 1, CAP), f32)
    sigma2[:, :N1] = (f32(1.2) ** (2 * rs.randint(0, 8, (NC + 1, N1)))).astype(f32)
    mp1 = np.arange(N1, dtype=np.int32)
    mp2, idx2 = np.full((NC, N1), -1, np.int32), np.full((NC, N1), -1, np.int32)
    for c in range(NC):
        R2, t2 = rot(rs, 0.3), rs.uniform(-1, 1, 3)
        R12, t12, s = rot(rs, 0.5), rs.uniform(-0.5, 0.5, 3), rs.uniform(0.5, 2.0)
        feat = np.sort(rs.permutation(N1)[:NMATCH])
        Xn = X1[feat].copy()
        Xn[:, :2] += rs.normal(0, 0.5, (NMATCH, 2)) * Xn[:, 2:3] / 517.0
        X2 = ((Xn - t12) @ R12) / s
        wrong = np.arange(NMATCH) if c >= n_true else rs.permutation(NMATCH)[:NMATCH // 5]
        X2[wrong] = np.stack([rs.uniform(-2, 2, len(wrong)), rs.uniform(-1.5, 1.5, len(wrong)), rs.uniform(3, 9, len(wrong)) / s], 1)
        mp2[c, feat] = N1 + c * NMATCH + np.arange(NMATCH)
        idx2[c, feat] = rs.permutation(N1)[:NMATCH]
        pos.append((X2 - t2) @ R2)
        cams[c + 1] = cam(R2, t2)
    return dict(cams=cams, pos=np.concatenate(pos).astype(f32), sigma2=sigma2, mp1=mp1, mp2=mp2, idx2=idx2)


def round_robin(solvers):
    """LoopClosing.cc:303-371 as far as the solver goes: iterate(5) over the live candidates until one answers or all are discarded"""
    live = list(range(len(solvers)))
    while live:
        for c in list(live):
            T, no_more, vb, n_in = solvers[c].iterate(5)
            if no_more:
                live.remove(c)
            if T is not None:
                return c, n_in
    return -1, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_sim3.py measures on the GPU: none found")
    from importlib import import_module
    sim3 = import_module("anyfeature-vslam_amd.sim3")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "sim3_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "sim3_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).sim3_host
    host.restype = None
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    words = (CAP + 31) // 32
    for label, n_true in (("all candidates false", 0), ("one candidate true", 1)):
        W = world(n_true)
        table = afv.table.DescriptorTable(ctx, NC + 1, CAP)
        points = afv.MapPoints(ctx, len(W["pos"]))
        ids = np.arange(len(W["pos"]), dtype=np.int32)
        points.set(ids, pos=W["pos"])
        zeros = np.zeros(N1, f32)
        for s in range(NC + 1):
            table.set(s, np.zeros((N1, 32), np.uint8))
            table.set_geometry(s, zeros, zeros, W["sigma2"][s, :N1])
        cands = list(range(1, NC + 1))
        seeds = [7 + c for c in range(NC)]

        def batch():
            sol = afv.Sim3Solver.batch(table, points, 0, cands, W["mp1"], W["mp2"], W["idx2"], W["cams"], False, seed=7, nhyp=NHYP)
            for s in sol:
                s.SetRansacParameters(0.99, MIN_INLIERS, NHYP)
            return sol
        solvers = batch()
        t_batch, t_call, t_scan, t_host, t_host_stop = [], [], [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            batch()
            t_batch.append(time.perf_counter() - t0)
        jobs = sim3.sim3_jobs(W["cams"][0], [W["cams"][c] for c in cands], False, seeds)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            out = sim3.hypotheses(table, points, [0] * NC, cands, jobs, W["mp1"], W["mp2"], W["idx2"], nhyp=NHYP)
            t_call.append(time.perf_counter() - t0)
        winner = None
        for _ in range(a.calls):
            for s in solvers:
                s.SetRansacParameters(0.99, MIN_INLIERS, NHYP)
                s.mnBestInliers, s.best = 0, None
            t0 = time.perf_counter()
            winner = round_robin(solvers)
            t_scan.append(time.perf_counter() - t0)
        # the host program over the same inputs
        camrec = np.zeros((NC, 32), f32)
        for c in range(NC):
            for o, cam in ((0, W["cams"][0]), (16, W["cams"][c + 1])):
                camrec[c, o:o + 9], camrec[c, o + 9:o + 12] = cam["Rcw"], cam["tcw"]
                camrec[c, o + 12:o + 16] = [cam["fx"], cam["fy"], cam["cx"], cam["cy"]]
        pad = lambda r: np.concatenate([r, np.full((NC, CAP - N1), -1, np.int32)], 1)
        mp1 = pad(np.broadcast_to(W["mp1"], (NC, N1)))
        mp2, idx2 = pad(W["mp2"]), pad(W["idx2"])
        idx1 = pad(np.broadcast_to(np.arange(N1, dtype=np.int32), (NC, N1)))
        s1 = np.ascontiguousarray(np.broadcast_to(W["sigma2"][0], (NC, CAP)))
        s2 = np.ascontiguousarray(W["sigma2"][1:])
        flags = np.ones(len(W["pos"]), np.uint8)
        useeds, n1s = np.array(seeds, np.uint64), np.full(NC, N1, np.int32)
        h = dict(n=np.zeros(NC, np.int32), index1=np.zeros((NC, CAP), np.int32), count=np.zeros((NC, NHYP), np.int32),
                 degenerate=np.zeros((NC, NHYP), np.uint8), sim3=np.zeros((NC, NHYP, 13), f32), inliers=np.zeros((NC, NHYP, words), np.uint32))

        def run_host(nhyp):
            host(NC, CAP, nhyp, words, 0, p_(camrec), p_(useeds), p_(n1s), p_(W["pos"]), p_(flags), p_(s1), p_(s2), p_(mp1), p_(mp2), p_(idx1), p_(idx2),
                 p_(h["n"]), p_(h["index1"]), p_(h["count"]), p_(h["degenerate"]), p_(h["sim3"]), p_(h["inliers"]))
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host(NHYP)
            t_host.append(time.perf_counter() - t0)
        same = all(h[k].tobytes() == out[k].tobytes() for k in h)
        # what the reference runs: every candidate up to the iteration at which the round-robin loop left it
        stop = max(s.mnIterations for s in solvers)
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host(stop)
            t_host_stop.append(time.perf_counter() - t0)
        run_host(NHYP)
        extra = dict(workload=label, candidates=NC, correspondences=float(np.mean(out["n"])), hypotheses=NHYP)
        stats("device: Sim3Solver.batch through the Python wrapper", t_batch, **extra)
        stats("device: afv_table_sim3_hypotheses alone, records built beforehand", t_call, equal_to_host_program=same, **extra)
        stats("host scan: the round-robin iterate(5) loop over the solvers (Python)", t_scan, winner=winner[0], inliers=winner[1],
              iterations_of_the_longest=stop, **extra)
        stats("host program: all %d hypotheses of every candidate" % NHYP, t_host, **extra)
        stats("host program: %d hypotheses per candidate, where the round-robin loop stopped" % stop, t_host_stop, **extra)
        points.close()
        table.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

"""Initializer on the device (afv_frame_initializer: three launches, the H and F RANSAC over every iteration and the reconstruction) next to
the same algorithm as a scalar host program (tools/initializer_host.cpp, g++ -O3 -ffp-contract=off, compiled here; ONE thread - the
reference spends two on the RANSAC half).  Two frames of 1000 features, 200 iterations, sigma 1; two workloads: 300 and 600 matches (a
cloud seen from two positions, 0.5 px of noise, 20 % gross outliers).  Host-to-host times over --calls calls each, median and
[fastest, slowest], one JSON line per figure:

  Initializer.Initialize through the Python wrapper (arrays made inside the clock)
  afv_frame_initializer alone, every array made beforehand (what a C++ caller pays), without and with the per-hypothesis outputs
  the host program over the same inputs (its own clock, inside the process)

The device's answers - outputs, trace, per-hypothesis arrays - are compared with the host program's, bit for bit, in the same run.

    python tools/time_initializer.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_initializer.py --calls 20
(k_init_prepare, k_init_hypotheses, k_init_reconstruct)"""
import argparse
import ctypes as C
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
f32 = np.float32
N_FEATURES, ITERATIONS, SEED = 1000, 200, 7
FX, FY, CX, CY, SIGMA = 517.3, 516.5, 318.6, 255.3, 1.0


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def world(n_match, seed=1):
    """two frames of N_FEATURES features; n_match of frame 1 are matched: a cloud 3 .. 8 m away seen after a small rotation and a 0.4 m
    step sideways, 0.5 px of noise, every fifth match a gross outlier; the other features are unrelated positions"""
    rs = np.random.RandomState(seed)
    z = rs.uniform(3, 8, n_match)
    P = np.stack([rs.uniform(-0.55, 0.55, n_match) * z, rs.uniform(-0.4, 0.4, n_match) * z, z], 1)
    a = 0.03
    Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Q = P @ Rm.T + np.array([0.4, 0.05, 0.03])
    proj = lambda X: (FX * X[:, 0] / X[:, 2] + CX + rs.normal(0, 0.5, len(X)), FY * X[:, 1] / X[:, 2] + CY + rs.normal(0, 0.5, len(X)))
    (u1, v1), (u2, v2) = proj(P), proj(Q)
    out = rs.choice(n_match, n_match // 5, replace=False)
    u2[out], v2[out] = rs.uniform(20, 620, len(out)), rs.uniform(20, 460, len(out))
    rest = N_FEATURES - n_match
    x1, y1 = np.concatenate([u1, rs.uniform(0, 640, rest)]), np.concatenate([v1, rs.uniform(0, 480, rest)])
    x2, y2 = np.concatenate([u2, rs.uniform(0, 640, rest)]), np.concatenate([v2, rs.uniform(0, 480, rest)])
    p1, p2 = rs.permutation(N_FEATURES), rs.permutation(N_FEATURES)
    X1, Y1, X2, Y2 = (np.zeros(N_FEATURES, f32) for _ in range(4))
    X1[p1], Y1[p1], X2[p2], Y2[p2] = x1, y1, x2, y2
    m = np.full(N_FEATURES, -1, np.int32)
    m[p1[:n_match]] = p2[:n_match]
    return X1, Y1, X2, Y2, m


def frame_of(afv, ctx, x, y):
    fr = afv.Frame(ctx, min_x=-4000.0, min_y=-4000.0, max_x=4000.0, max_y=4000.0)
    kps = np.zeros(len(x), afv.KP_DTYPE)
    kps["x"], kps["y"] = x, y
    fr.set_features(kps, np.zeros((len(x), 32), np.uint8), sizes=np.ones(len(x), f32))
    return fr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    afv = importlib.import_module("anyfeature-vslam_amd")
    ini = importlib.import_module("anyfeature-vslam_amd.initializer")
    L = afv._lib
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(tmp.name, "initializer_host")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "initializer_host.cpp"), "-o", exe], check=True)
    words = (N_FEATURES + 31) // 32
    for n_match in (300, 600):
        x1, y1, x2, y2, m = world(n_match)
        f1, f2 = frame_of(afv, ctx, x1, y1), frame_of(afv, ctx, x2, y2)
        job = L.sized(L.InitJob)
        job.iterations, job.seed_lo, job.seed_hi = ITERATIONS, SEED, 0
        job.fx, job.fy, job.cx, job.cy, job.sigma = FX, FY, CX, CY, SIGMA
        full = ini.initialize(f1, f2, job, m, hypotheses=True)
        # the host program over the same inputs
        scene, answer = os.path.join(tmp.name, "scene.bin"), os.path.join(tmp.name, "answer.bin")
        with open(scene, "wb") as f:
            f.write(struct.pack("<4iQ5f", N_FEATURES, N_FEATURES, ITERATIONS, a.calls, SEED, FX, FY, CX, CY, SIGMA))
            for arr in (x1, y1, x2, y2):
                f.write(np.ascontiguousarray(arr, f32).tobytes())
            f.write(m.tobytes())
        r = subprocess.run([exe, scene, answer], capture_output=True, text=True, check=True)
        host_ms = [float(v) for v in r.stdout.split()]
        tr = full["trace"]
        mine = b"".join([struct.pack("<2i", full["ok"], full["route"]), full["R21"].tobytes(), full["t21"].tobytes(), full["p3d"].tobytes(),
                         full["triangulated"].tobytes(), bytes(tr), full["score"].tobytes(), full["model"].tobytes(), full["degenerate"].tobytes(),
                         full["inliers"].tobytes()])
        assert full["inliers"].shape[2] == words
        same = mine == open(answer, "rb").read()
        # Initializer.Initialize through the Python wrapper
        K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], f32)
        init = afv.Initializer(f1, K, SIGMA, ITERATIONS)
        t_class, t_call, t_call_hyp = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            init.Initialize(f2, m, seed=SEED)
            t_class.append(time.perf_counter() - t0)
        # afv_frame_initializer alone
        lib = L.load()
        ok, route = C.c_int32(0), C.c_int32(0)
        R21, t21, p3d, tri = np.zeros(9, f32), np.zeros(3, f32), np.zeros((N_FEATURES, 3), f32), np.zeros(N_FEATURES, np.uint8)
        trace = L.sized(L.InitTrace)
        sc, mo, dg = np.zeros((2, ITERATIONS), f32), np.zeros((2, ITERATIONS, 9), f32), np.zeros((2, ITERATIONS), np.uint8)
        inl = np.zeros((2, ITERATIONS, words), np.uint32)
        p_ = L.ptr
        for with_hyp, sink in ((False, t_call), (True, t_call_hyp)):
            hyp = (p_(sc), p_(mo), p_(dg), p_(inl)) if with_hyp else (None, None, None, None)
            for _ in range(a.calls):
                t0 = time.perf_counter()
                rc = lib.afv_frame_initializer(f1.handle, f2.handle, C.byref(job), p_(m), C.byref(ok), C.byref(route), p_(R21), p_(t21), p_(p3d),
                                               p_(tri), C.byref(trace), *hyp, words)
                sink.append(time.perf_counter() - t0)
                assert rc == 0
        extra = dict(features=N_FEATURES, matches=n_match, iterations=ITERATIONS, ok=full["ok"], route="HF"[full["route"]],
                     reason=L.INIT_REASON[tr.reason], inliers=tr.n_inliers)
        stats("device: Initializer.Initialize through the Python wrapper", t_class, **extra)
        stats("device: afv_frame_initializer alone, arrays made beforehand", t_call, **extra)
        stats("device: afv_frame_initializer alone, with the per-hypothesis outputs", t_call_hyp, equal_to_host_program=same, **extra)
        print(json.dumps(dict({"path": "host program (one thread): tools/initializer_host.cpp", "host_to_host_ms_median": host_ms[0],
                               "ms_min": host_ms[1], "ms_max": host_ms[2]}, **extra)), flush=True)
        assert same, "the device and the host program disagree"
        f1.close()
        f2.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

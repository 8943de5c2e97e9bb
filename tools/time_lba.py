"""LocalBundleAdjustment on the device (afv_table_bundle_adjust: the host drives the Levenberg loop, a handful of launches and one wait per
trial) next to the same algorithm as a scalar host program (tools/lba_host.cpp, g++ -O3 -ffp-contract=off, compiled here).  Two
workloads: 10 free + 10 fixed keyframes and 40 free + 40 fixed, about 100 points per keyframe, every point seen by four keyframes, 10 %
of the observations gross outliers, 0.5 px of noise, a start a few centimetres off.  write_points = 0, so every call starts from the same
store.  Host-to-host times over --calls calls each, median with [fastest, slowest], one JSON line per figure:

  afv_table_bundle_adjust, edge arrays and records built beforehand (what a C++ caller pays)
  the host program over the same inputs (observations gathered beforehand)

The device's answers are compared with the host program's, bit for bit, once per workload.

    python tools/time_lba.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_lba.py --calls 20
(k_lba_*)"""
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
FX, FY, CX, CY, BF = 517.3, 516.5, 318.6, 255.3, 40.0
VIEWS, PER_KF = 4, 100


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def world(n_free, n_fixed, seed=1):
    """keyframes on a line looking along z (free and fixed interleaved in space), point p seen by VIEWS neighbouring keyframes"""
    rs = np.random.RandomState(seed)
    nk = n_free + n_fixed
    npts = nk * PER_KF // VIEWS
    place = rs.permutation(nk)                                   # keyframe k stands at position place[k] of the line
    cams = np.zeros((nk, 17), np.float64)
    for k in range(nk):
        a = 0.01 * (place[k] - nk / 2.0)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        cams[k, :9], cams[k, 9:12] = R.reshape(9), -R @ np.array([0.15 * place[k], 0.01 * (k % 5), 0.0])
        cams[k, 12:17] = (FX, FY, CX, CY, BF)
    cams = cams.astype(f32)
    at = np.argsort(place)                                       # at[i]: the keyframe at position i
    feats = [dict(x=[], y=[], ur=[], inf=[]) for _ in range(nk)]
    X = np.zeros((npts, 3))
    e_pt, e_kf, e_idx = [], [], []
    for p in range(npts):
        first = rs.randint(0, nk - VIEWS + 1)
        X[p] = [0.15 * (first + 1.5) + rs.uniform(-1.5, 1.5), rs.uniform(-1, 1), rs.uniform(4, 9)]
        for i in range(first, first + VIEWS):
            k = int(at[i])
            c = cams[k].astype(np.float64)
            q = c[:9].reshape(3, 3) @ X[p] + c[9:12]
            u, v = FX * q[0] / q[2] + CX + rs.normal(0, 0.5), FY * q[1] / q[2] + CY + rs.normal(0, 0.5)
            if rs.uniform() < 0.1:
                u += rs.choice([-1, 1]) * rs.uniform(15, 60)
            f = feats[k]
            e_pt.append(p); e_kf.append(k); e_idx.append(len(f["x"]))
            f["x"].append(u); f["y"].append(v); f["ur"].append(-1.0); f["inf"].append(1.0 / 1.2 ** (2 * rs.randint(0, 8)))
    start = cams.copy()
    start[:n_free, 9:12] += rs.normal(0, 0.01, (n_free, 3)).astype(f32)
    return dict(nk=nk, nf=n_free, np=npts, cams=start, pos=(X + rs.normal(0, 0.03, X.shape)).astype(f32),
                feats=[{n: np.asarray(v, f32) for n, v in f.items()} for f in feats],
                e_pt=np.asarray(e_pt, np.int32), e_kf=np.asarray(e_kf, np.int32), e_idx=np.asarray(e_idx, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_lba.py measures on the GPU: none found")
    lba = importlib.import_module("anyfeature-vslam_amd.lba")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "lba_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "anyfeature-vslam_amd", "csrc"), "-shared", "-fPIC",
                    os.path.join(ROOT, "tools", "lba_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).lba_host
    host.restype = None
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    for n_free, n_fixed in ((10, 10), (40, 40)):
        W = world(n_free, n_fixed)
        nk, npts, ne = W["nk"], W["np"], len(W["e_pt"])
        cap = max(len(f["x"]) for f in W["feats"])
        table = afv.table.DescriptorTable(ctx, nk, cap)
        points = afv.MapPoints(ctx, npts)
        ids = np.arange(npts, dtype=np.int32)
        points.set(ids, pos=W["pos"])
        for k, f in enumerate(W["feats"]):
            n = len(f["x"])
            table.set(k, np.zeros((n, 32), np.uint8))
            table.set_geometry(k, f["x"], f["y"], np.ones(n, f32), u_right=f["ur"])
            table.set_inf(k, f["inf"])
        recs = lba.lba_cams([dict(Rcw=c[:9], tcw=c[9:12], fx=c[12], fy=c[13], cx=c[14], cy=c[15], mbf=c[16]) for c in W["cams"]])
        slots = np.arange(nk, dtype=np.int32)
        call = lambda: lba.bundle_adjust(table, points, slots, n_free, recs, ids, W["e_pt"], W["e_kf"], W["e_idx"], (5, 10), (1, 0), 1, write_points=False)
        res, kf, xyz, state = call()
        t_call, t_host = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            t_call.append(time.perf_counter() - t0)
        obs = np.zeros((ne, 4), f32)
        for e in range(ne):
            f = W["feats"][W["e_kf"][e]]
            obs[e] = (f["x"][W["e_idx"][e]], f["y"][W["e_idx"][e]], f["ur"][W["e_idx"][e]], f["inf"][W["e_idx"][e]])
        params = np.array([5, 10, 1, 0, 1, -1], np.int32)
        ok = np.ones(npts, np.uint8)
        ints, dbl, hkf, hxyz, hstate = np.zeros(8, np.int32), np.zeros(4), np.zeros((n_free, 12)), np.zeros((npts, 3)), np.zeros(ne, np.uint8)
        cams_f, pos_f = np.ascontiguousarray(W["cams"]), np.ascontiguousarray(W["pos"])

        def run_host():
            host(nk, n_free, npts, ne, p_(cams_f), p_(pos_f), p_(ok), p_(W["e_pt"]), p_(W["e_kf"]), p_(obs), p_(params), p_(ints), p_(dbl), p_(hkf),
                 p_(hxyz), p_(hstate))
        for _ in range(a.calls):
            t0 = time.perf_counter()
            run_host()
            t_host.append(time.perf_counter() - t0)
        same = [*res.iterations, *res.trials, res.n_edges, res.n_removed_first, res.n_erase, res.stopped] == list(ints)
        same &= np.array(list(res.chi2) + list(res.lam)).tobytes() == dbl.tobytes()
        same &= kf.tobytes() == hkf.tobytes() and xyz.tobytes() == hxyz.tobytes() and bool(np.array_equal(state, hstate))
        extra = dict(free=n_free, fixed=n_fixed, points=npts, edges=ne, iterations=sum(res.iterations), trials=sum(res.trials),
                     removed_first=res.n_removed_first, erase=res.n_erase)
        stats("device: afv_table_bundle_adjust, records built beforehand", t_call, equal_to_host_program=bool(same), **extra)
        stats("host program: tools/lba_host.cpp", t_host, **extra)
        points.close()
        table.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

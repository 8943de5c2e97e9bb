"""Tracking::SearchLocalPoints through resident map points (afv_frame_search_points: point ids in, one launch for the geometry and the
descriptor gather) next to the path an integrator had before it: Frame::isInFrustum and the radius for every point on the host - once as
the C++ loop of tools/points_host_loop.cpp (compiled here with g++), once as vectorised numpy, the same float statements both times - then
afv_frame_match_projection with the descriptors by reference (qref_table).  One 640 x 480
frame of about 1000 features; 1000 and 2000 map points made from its keypoints at random depths, some outside the frustum.  Host-to-host
times over --calls calls each, median and spread; the two paths' answers are compared.  Also the cost of one launch on this machine: a
one-element torch kernel, launch to completion.  One JSON line per figure.

    python tools/time_points.py [--calls 300]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_points.py --calls 20  (k_points_project)"""
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
FX, FY, CX, CY, MBF = 500.0, 500.0, 320.0, 240.0, 40.0
RADIUS_TH, COS_LIMIT, SCALE = 3.0, 0.5, 1.15


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def frustum_on_host(w, Rcw, tcw, Ow, tol):
    """Frame::isInFrustum + the radius of SearchByProjection(F, vpMapPoints) over arrays: the float statements of the device kernel, in its
    order, one numpy operation each (no fused multiply-add)"""
    with np.errstate(all="ignore"):
        X, Y, Z = w["pos"][:, 0], w["pos"][:, 1], w["pos"][:, 2]
        pc = [Rcw[k, 0] * X + (Rcw[k, 1] * Y + Rcw[k, 2] * Z) + tcw[k] for k in range(3)]
        invz = f32(1.0) / pc[2]
        u = (f32(FX) * pc[0]) * invz + f32(CX)
        v = (f32(FY) * pc[1]) * invz + f32(CY)
        ok = ~(pc[2] < 0) & ~(u < 0) & ~(u > 640) & ~(v < 0) & ~(v > 480)
        p0, p1, p2 = X - Ow[0], Y - Ow[1], Z - Ow[2]
        dist = np.sqrt(p0 * p0 + (p1 * p1 + p2 * p2))
        ok &= ~(dist < f32(0.8) * w["min"]) & ~(dist > f32(1.2) * w["max"])
        dot = p0 * w["normal"][:, 0] + (p1 * w["normal"][:, 1] + p2 * w["normal"][:, 2])
        vcos = dot / dist
        ok &= ~(vcos < f32(COS_LIMIT))
        size = (w["ref_size"] * w["ref_dist"]) / dist
        sigma = (w["ref_sigma"] * w["ref_dist"]) / dist
        by_cos = np.where(vcos.astype(np.float64) > 0.998, f32(2.5), f32(4.0)).astype(np.float32)
        r = ((f32(SCALE) * f32(RADIUS_TH)) * by_cos) * size
        qmin, qmax = size / tol, size * tol
        ok &= np.isfinite(u) & np.isfinite(v) & np.isfinite(r) & np.isfinite(qmin) & np.isfinite(qmax)
        ur = u - f32(MBF) * invz
        return ok, u, v, r, qmin, qmax, ur, r * sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_points.py measures on the GPU: none found")
    ctx = afv.Context()
    frame = afv.Frame(ctx)
    kps, desc = frame.extract(afv.synth.corners_frame(1))
    n = len(kps)
    sizes = ctx.size_sigma(kps)[0]
    Rcw, tcw = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    Ow = np.zeros(3, np.float32)
    frame.set_pose(Rcw, tcw, Ow, FX, FY, CX, CY, MBF)
    table = afv.table.DescriptorTable(ctx, 1, max(n, 1))
    table.set(0, desc, kps["angle"])
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    m = afv.FeatureMatcher(0.8, False, ctx=ctx)
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "points_host_loop.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "points_host_loop.cpp"), "-o", so],
                   check=True)
    loop = C.CDLL(so).points_host_loop
    loop.restype = C.c_int
    host_point = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min", "<f4"), ("max", "<f4"), ("ref_size", "<f4"), ("ref_dist", "<f4"),
                           ("ref_sigma", "<f4")])
    ptr = afv._lib.ptr
    # the cost of a launch here: a one-element kernel, launch to completion
    x = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    lt = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        x.add_(1.0)
        torch.cuda.synchronize()
        lt.append(time.perf_counter() - t0)
    stats("one-element kernel: launch to completion", lt)
    for nq in (1000, 2000):
        rs = np.random.RandomState(nq)
        src = rs.randint(0, n, nq)                      # the keypoint a map point was made from
        z = rs.uniform(2.0, 10.0, nq).astype(np.float32)
        z[rs.rand(nq) < 0.1] *= -1                      # behind the camera
        px = kps["x"][src] + rs.uniform(-2, 2, nq) + np.where(rs.rand(nq) < 0.15, 700.0, 0.0)   # some outside the image
        py = kps["y"][src] + rs.uniform(-2, 2, nq)
        pos = np.stack([(px - CX) / FX * z, (py - CY) / FY * z, z], 1).astype(np.float32)
        dist = np.linalg.norm(pos, axis=1).astype(np.float32)
        w = {"pos": pos, "normal": (pos / dist[:, None]).astype(np.float32), "min": dist * f32(0.7), "max": dist * f32(1.3),
             "ref_size": sizes[src].astype(np.float32), "ref_dist": dist, "ref_sigma": np.full(nq, 0.5, np.float32)}
        ids = rs.permutation(4096)[:nq].astype(np.int32)
        points = afv.MapPoints(ctx, 4096)
        points.set(ids, pos=w["pos"], normal=w["normal"], min_distance=w["min"], max_distance=w["max"], ref_size=w["ref_size"],
                   ref_distance=w["ref_dist"], ref_sigma=w["ref_sigma"])
        points.set_flags(ids, bad=np.zeros(nq), observed=np.ones(nq))
        slots, idx = np.zeros(nq, np.int32), src.astype(np.int32)
        points.set_descriptors_from_table(ids, table, slots, idx)
        tol = f32(ctx.params.scale_factor)

        zero_rows = np.zeros((nq, 32), np.uint8)   # (the rows come by reference)

        def path_a():
            t0 = time.perf_counter()
            ok, u, v, r, qmin, qmax, ur, er = frustum_on_host(w, Rcw, tcw, Ow, tol)
            q = afv.ProjectionQueries(zero_rows, u, v, r, qmin, qmax, valid=ok, ur=ur, er_max=er)
            t1 = time.perf_counter()
            got = frame.SearchByProjection(m, q, qref=(table, slots, idx))
            return got, int(ok.sum()), t1 - t0, time.perf_counter() - t1

        hp = np.zeros(nq, host_point)
        for k in host_point.names:
            hp[k] = w[k]
        cu, cv, cr, cmin, cmax, cur, cer = (np.zeros(nq, np.float32) for _ in range(7))
        cok = np.zeros(nq, np.uint8)
        fl = C.c_float

        def path_c():
            """the same with the C++ loop building the queries"""
            t0 = time.perf_counter()
            nin = loop(ptr(hp), nq, ptr(Rcw), ptr(tcw), ptr(Ow), fl(FX), fl(FY), fl(CX), fl(CY), fl(MBF), fl(0.0), fl(640.0), fl(0.0), fl(480.0),
                       fl(float(f32(SCALE) * f32(RADIUS_TH))), fl(COS_LIMIT), fl(float(tol)), ptr(cok), ptr(cu), ptr(cv), ptr(cr), ptr(cmin), ptr(cmax),
                       ptr(cur), ptr(cer))
            q = afv.ProjectionQueries(zero_rows, cu, cv, cr, cmin, cmax, valid=cok, ur=cur, er_max=cer)
            t1 = time.perf_counter()
            got = frame.SearchByProjection(m, q, qref=(table, slots, idx))
            return got, int(nin), t1 - t0, time.perf_counter() - t1

        def path_b():
            t0 = time.perf_counter()
            got = frame.SearchLocalPoints(m, points, ids, RADIUS_TH, COS_LIMIT)
            return got, time.perf_counter() - t0

        (ga, na), in_view_a, _, _ = path_a()
        (gb, nb, in_view_b), _ = path_b()
        (gc, nc), in_view_c, _, _ = path_c()
        same = bool(na == nb == nc and np.array_equal(ga, gb) and np.array_equal(gc, gb) and in_view_a == in_view_c == int(in_view_b.sum()))
        build, search, total, dev = [], [], [], []
        cbuild, csearch, ctotal = [], [], []
        for _ in range(a.calls):
            _, _, tb, ts = path_a()
            build.append(tb); search.append(ts); total.append(tb + ts)
        for _ in range(a.calls):
            _, _, tb, ts = path_c()
            cbuild.append(tb); csearch.append(ts); ctotal.append(tb + ts)
        for _ in range(a.calls):
            dev.append(path_b()[1])
        med = lambda t: 1e3 * sorted(t)[len(t) // 2]
        stats("(a) numpy isInFrustum + afv_frame_match_projection(qref_table), nq=%d" % nq, total, host_build_ms_median=med(build),
              search_ms_median=med(search), matches=int(na), in_view=in_view_a, features=n)
        stats("(a) C++ loop isInFrustum + afv_frame_match_projection(qref_table), nq=%d" % nq, ctotal, host_build_ms_median=med(cbuild),
              search_ms_median=med(csearch), matches=int(nc), in_view=in_view_c)
        stats("(b) afv_frame_search_points, nq=%d" % nq, dev, matches=int(nb), in_view=int(in_view_b.sum()), equal_answers=same,
              minus_search_of_a_ms=med(dev) - min(med(search), med(csearch)))
        points.close()
    tmp.cleanup()
    table.close()
    frame.close()
    ctx.close()


if __name__ == "__main__":
    main()

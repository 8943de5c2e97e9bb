"""Fuse into keyframes of the table on the device (afv_table_fuse_points: one upload, geometry + membership, the search, the occupants, one
wait) next to the route a caller has without it: per target keyframe the projection loop of Fuse as scalar host code (tools/kffuse_host.cpp,
g++ -O3 -ffp-contract=off: FeatureMatcher.cc:811-858 and IsInKeyFrame) over the host's copy of the map, then ONE batched afv_match_fuse over
the host-array jobs - which uploads every keyframe's descriptors and geometry again - and the occupant lookup in the host's mvpMapPoints.
Two workloads:

  (a) 20 target keyframes of 1000 features, one shared list of 1000 points: the first half of LocalMapping::SearchInNeighbors
  (b) 1 target keyframe of 1000 features, 20 000 candidates: its second half (vpFuseCandidates into the current keyframe)

Host-to-host times over --calls calls each, the two routes alternating in one run, median with [fastest, slowest], one JSON line per
figure.  The answers of the two routes (best, occupant, status) are compared once per workload, bit for bit.

    python tools/time_kffuse.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_kffuse.py --calls 20
(k_kffuse_project, k_match_fuse, k_kffuse_finish, k_frame_grid; the host route's kernels are k_frame_grid and k_match_fuse)"""
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
W, H, FX, FY, CX, CY = 640.0, 480.0, 500.0, 500.0, 320.0, 240.0
TH_LOW = 50.0


class HostStore(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("normal", C.c_void_p), ("min_d", C.c_void_p), ("max_d", C.c_void_p), ("ref_size", C.c_void_p),
                ("ref_dist", C.c_void_p), ("flags", C.c_void_p), ("capacity", C.c_int32)]


class HostCamera(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("mbf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("rs_th", C.c_float), ("tol", C.c_float)]


def host_library():
    path = os.path.join(ROOT, "tools", "libkffuse_host.so")
    if not os.path.exists(path):  # a tree whose build() did not run: compile it next to the temporary files
        path = os.path.join(tempfile.mkdtemp(prefix="kffuse_"), "libkffuse_host.so")
        subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tools", "kffuse_host.cpp"), "-o", path],
                       check=True)
    lib = C.CDLL(path)
    lib.kffuse_host_project.restype = None
    lib.kffuse_host_project.argtypes = [C.POINTER(HostStore), C.POINTER(HostCamera), C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    return lib


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def world(npts, nk, nfeat, seed=1):
    """nk keyframes on a short line looking down +z, npts points in front of them; every keyframe's features sit near the projections of
    points (rows a few bits away) or anywhere; a third of the features already hold a point"""
    rs = np.random.RandomState(seed)
    z = rs.uniform(3.0, 9.0, npts)
    pos = np.stack([rs.uniform(-0.7, 0.7, npts) * z, rs.uniform(-0.5, 0.5, npts) * z, z], 1).astype(f32)
    dist = np.linalg.norm(pos, axis=1).astype(f32)
    w = dict(npts=npts, nk=nk, nfeat=nfeat, pos=pos, normal=(pos / dist[:, None]).astype(f32), min_d=(dist * f32(0.5)).astype(f32),
             max_d=(dist * f32(1.8)).astype(f32), ref_size=rs.choice([1.0, 1.2, 1.44], npts).astype(f32), ref_dist=dist.copy(),
             rows=rs.randint(0, 256, (npts, 32)).astype(np.uint8), flags=np.where(rs.rand(npts) < 0.03, 3, 1).astype(np.uint8), kfs=[])
    for k in range(nk):
        t = np.array([0.04 * k - 0.4, 0.01 * (k % 3), 0.0], f32)
        pc = pos + t
        u, v = f32(FX) * pc[:, 0] / pc[:, 2] + f32(CX), f32(FY) * pc[:, 1] / pc[:, 2] + f32(CY)
        inside = np.flatnonzero((u > 0) & (u < W) & (v > 0) & (v < H))
        owner = inside[rs.randint(0, len(inside), nfeat)]
        near = rs.rand(nfeat) < 0.7
        x = np.where(near, u[owner] + rs.uniform(-2, 2, nfeat), rs.uniform(0, W, nfeat)).astype(f32)
        y = np.where(near, v[owner] + rs.uniform(-2, 2, nfeat), rs.uniform(0, H, nfeat)).astype(f32)
        size = (w["ref_size"][owner] * w["ref_dist"][owner] / np.linalg.norm(pc[owner], axis=1)).astype(f32)
        rows = w["rows"][owner].copy()
        rows[np.arange(nfeat), rs.randint(0, 32, nfeat)] ^= np.uint8(1) << rs.randint(0, 8, nfeat).astype(np.uint8)
        rows[~near] = rs.randint(0, 256, (int((~near).sum()), 32))
        plane = np.where(rs.rand(nfeat) < 0.33, rs.randint(0, npts, nfeat), -1).astype(np.int32)
        w["kfs"].append(dict(t=t, x=x, y=y, size=size, rows=np.ascontiguousarray(rows), plane=plane, inf=(f32(1.0) / (size * size)).astype(f32)))
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    afv = importlib.import_module("anyfeature-vslam_amd")
    L = afv._lib
    host = host_library()
    ctx = afv.Context(max_width=1280, max_height=720, max_batch=1)
    afv.FeatureMatcher.setDescriptorDistanceThresholds(TH_LOW)
    matcher = afv.FeatureMatcher(0.8, False, ctx=ctx)
    tol = f32(1.2)
    inv_w, inv_h = f32(64) / f32(W), f32(48) / f32(H)
    for label, npts, nk, nfeat in (("20 targets x 1000 features, 1000 shared points", 1000, 20, 1000),
                                   ("1 target x 1000 features, 20000 candidates", 20000, 1, 1000)):
        w = world(npts, nk, nfeat)
        ids = np.arange(npts, dtype=np.int32)
        # ---- the device route: everything resident
        store = afv.MapPoints(ctx, npts)
        store.set(ids, pos=w["pos"], normal=w["normal"], min_distance=w["min_d"], max_distance=w["max_d"], ref_size=w["ref_size"],
                  ref_distance=w["ref_dist"], ref_sigma=np.ones(npts, f32))
        store.set_flags(ids, bad=w["flags"] & 2, observed=np.ones(npts, np.uint8))
        store.set_descriptors(ids, w["rows"])
        table = afv.table.DescriptorTable(ctx, nk, nfeat)
        table.set_camera(0.0, W, 0.0, H, 64, 48, inv_w, inv_h)
        eye = np.eye(3, dtype=f32)
        for k, kf in enumerate(w["kfs"]):
            table.set(k, kf["rows"])
            table.set_geometry(k, kf["x"], kf["y"], kf["size"] * kf["size"])
            table.set_scale(k, kf["size"])
            table.set_inf(k, kf["inf"])
            table.set_pose(k, eye, kf["t"], -kf["t"], FX, FY, CX, CY, 0.0)
            table.set_map_points(k, kf["plane"])
        targets = list(range(nk))

        def device():
            return table.FusePoints(store, targets, ids, radiusTh=3.0, th_low=TH_LOW)

        # ---- the host route: scalar projection per target, one batched afv_match_fuse, occupants from the host's planes
        hs = HostStore(L.ptr(w["pos"]), L.ptr(w["normal"]), L.ptr(w["min_d"]), L.ptr(w["max_d"]), L.ptr(w["ref_size"]), L.ptr(w["ref_dist"]),
                       L.ptr(w["flags"]), npts)
        cams, views, queries, status = [], [], [], []
        for kf in w["kfs"]:
            c = HostCamera()
            for i in range(9):
                c.R[i] = float(eye.reshape(9)[i])
            for i in range(3):
                c.t[i], c.Ow[i] = float(kf["t"][i]), float(-kf["t"][i])
            c.fx, c.fy, c.cx, c.cy, c.mbf, c.min_x, c.max_x, c.min_y, c.max_y = FX, FY, CX, CY, 0.0, 0.0, W, 0.0, H
            c.rs_th, c.tol = float(f32(1.15) * f32(3.0)), float(tol)
            cams.append(c)
            views.append(afv.FrameGridView(kf["rows"], np.stack([kf["x"], kf["y"]], 1), kf["size"], max_x=W, max_y=H, size_tolerance=float(tol),
                                           inf=kf["inf"], u_right=np.full(nfeat, -1, f32)))
            z = lambda: np.zeros(npts, f32)
            queries.append(afv.ProjectionQueries(np.zeros((npts, 32), np.uint8), z(), z(), z(), z(), z(), valid=np.zeros(npts, np.uint8), ur=z()))
            status.append(np.zeros(npts, np.uint8))
        jobs = (L.ProjJob * nk)()
        best = np.full(nk * npts, -1, np.int32)
        nfound = np.zeros(nk, np.int32)

        def host_route():
            rows = w["rows"][ids]                                   # the descriptors of the list, gathered once for all targets
            for k in range(nk):
                q = queries[k]
                host.kffuse_host_project(C.byref(hs), C.byref(cams[k]), L.ptr(ids), npts, L.ptr(w["kfs"][k]["plane"]), nfeat, L.ptr(q.u), L.ptr(q.v),
                                         L.ptr(q.r), L.ptr(q.min_size), L.ptr(q.max_size), L.ptr(q.ur), L.ptr(q.valid), L.ptr(status[k]))
                q.descriptors = rows
                j = matcher._proj_job(views[k], q)
                j.th_high = TH_LOW
                jobs[k] = j
            ctx.check(ctx.lib.afv_match_fuse(ctx.handle, jobs, nk, L.ptr(best), L.ptr(nfound)), "afv_match_fuse")
            out = []
            for k in range(nk):
                b = best[k * npts:(k + 1) * npts]
                plane = w["kfs"][k]["plane"]
                occ = np.where(b >= 0, plane[np.clip(b, 0, None)], -1).astype(np.int32)
                st = status[k].copy()
                pending = st == 255
                bad_occ = (occ >= 0) & ((w["flags"][np.clip(occ, 0, None)] & 2) != 0)
                st[pending] = np.where(b[pending] < 0, 3, np.where(occ[pending] < 0, 4, np.where(bad_occ[pending], 5, 6)))
                out.append((b.copy(), occ, st))
            return out

        d = device()
        h = host_route()
        same = all(np.array_equal(d[0][k], h[k][0]) and np.array_equal(d[1][k], h[k][1]) and np.array_equal(d[2][k], h[k][2]) for k in range(nk))
        counts = np.bincount(np.concatenate(d[2]), minlength=7).tolist()
        t_dev, t_host = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter(); device(); t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); host_route(); t_host.append(time.perf_counter() - t0)
        stats("afv_table_fuse_points: " + label, t_dev, answers_equal=bool(same), status_counts=counts, nfused=int(sum(d[3])))
        stats("host projection + batched afv_match_fuse: " + label, t_host)
        # the projection loop alone, per call
        t_proj = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            for k in range(nk):
                q = queries[k]
                host.kffuse_host_project(C.byref(hs), C.byref(cams[k]), L.ptr(ids), npts, L.ptr(w["kfs"][k]["plane"]), nfeat, L.ptr(q.u), L.ptr(q.v),
                                         L.ptr(q.r), L.ptr(q.min_size), L.ptr(q.max_size), L.ptr(q.ur), L.ptr(q.valid), L.ptr(status[k]))
            t_proj.append(time.perf_counter() - t0)
        stats("  of which the scalar projection loop: " + label, t_proj)
        table.close()
        store.close()
        if not same:
            raise SystemExit("the two routes disagree")
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)


if __name__ == "__main__":
    main()

"""ComputeDistinctiveDescriptors + UpdateNormalAndDepth of resident map points on the device (afv_table_refresh_points: one upload, one
launch per part, one wait) next to the route a host has without it: tools/refresh_host.cpp (g++ -O3 -ffp-contract=off, compiled here)
does the normal part over the host's copy of the map, afv_distinctive_descriptors chooses the rows from host arrays gathered out of the
keyframes' descriptors, and afv_points_set + afv_points_set_descriptors_from_table upload the result; the route ends when the device has
taken it (a device synchronise).  Two workloads:

  (a) 1000 points x 8 observations over 20 keyframes, both parts: the end of LocalMapping::SearchInNeighbors
  (b) 2000 points x 4 observations over 80 keyframes, the normal part alone: after a local bundle adjustment

Host-to-host times over --calls calls each, median with [fastest, slowest], one JSON line per figure.  Both routes start from the same
store; their answers (every plane and row of the store, the chosen observations) are compared once per workload, bit for bit.

    python tools/time_refresh.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_refresh.py --calls 20
(k_refresh_desc, k_refresh_normals; the host route's kernels are k_distinctive, k_points_move, k_points_rows)"""
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


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def world(npts, views, nk, seed=1):
    """keyframes on a line; point p is seen by `views` neighbouring keyframes, one feature each; rows random"""
    rs = np.random.RandomState(seed)
    n = [0] * nk
    obs_kf, obs_idx = np.zeros((npts, views), np.int32), np.zeros((npts, views), np.int32)
    for p in range(npts):
        first = rs.randint(0, nk - views + 1)
        for v in range(views):
            obs_kf[p, v], obs_idx[p, v] = first + v, n[first + v]
            n[first + v] += 1
    cap = max(n)
    return dict(nk=nk, np=npts, views=views, cap=cap, n=n, obs_kf=obs_kf.reshape(-1), obs_idx=obs_idx.reshape(-1),
                obs_point=np.repeat(np.arange(npts, dtype=np.int32), views), rows=rs.randint(0, 256, (nk, cap, 32)).astype(np.uint8),
                size=(f32(31.0) * f32(1.2) ** rs.randint(0, 8, (nk, cap))).astype(f32), sigma2=(f32(1.44) ** rs.randint(0, 8, (nk, cap))).astype(f32),
                centres=np.stack([0.15 * np.arange(nk), 0.01 * (np.arange(nk) % 5), np.zeros(nk)], 1).astype(f32),
                max_size=np.full(nk, f32(31.0) * f32(1.2) ** 7, f32), ref=obs_kf[:, 0].copy(),
                pos=np.stack([rs.uniform(-1.5, 4.5, npts), rs.uniform(-1, 1, npts), rs.uniform(4, 9, npts)], 1).astype(f32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_refresh.py measures on the GPU: none found")
    refresh = importlib.import_module("anyfeature-vslam_amd.refresh")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "refresh_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "refresh_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).refresh_host
    host.restype = None
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    for label, npts, views, nk, descriptors in (("a", 1000, 8, 20, True), ("b", 2000, 4, 80, False)):
        W = world(npts, views, nk)
        ne = npts * views
        table = afv.table.DescriptorTable(ctx, nk, W["cap"])
        for k in range(nk):
            m = W["n"][k]
            table.set(k, W["rows"][k, :m])
            table.set_geometry(k, np.zeros(m, f32), np.zeros(m, f32), W["sigma2"][k, :m])
            table.set_scale(k, W["size"][k, :m])
        ids, slots = np.arange(npts, dtype=np.int32), np.arange(nk, dtype=np.int32)
        stale = dict(pos=W["pos"], normal=np.zeros((npts, 3), f32), min_distance=np.ones(npts, f32), max_distance=np.ones(npts, f32),
                     ref_size=np.ones(npts, f32), ref_distance=np.ones(npts, f32), ref_sigma=np.ones(npts, f32))
        stores = []
        for _ in range(2):
            s = afv.MapPoints(ctx, npts)
            s.set(ids, **stale)
            s.set_descriptors(ids, np.zeros((npts, 32), np.uint8))
            stores.append(s)
        dev, via_host = stores
        call = lambda: refresh.refresh_points(table, dev, slots, W["centres"], W["max_size"], None, ids, W["ref"], W["obs_point"], W["obs_kf"],
                                              W["obs_idx"], descriptors, True)
        status, best, med = call()
        # the host's route: its own copy of the map (positions, flags), the keyframes' descriptors as they lie in mDescriptors
        pt_ptr = (np.arange(npts + 1) * views).astype(np.int32)
        flags = np.ones(npts, np.uint8)
        h = {k: np.ascontiguousarray(v).copy() for k, v in stale.items()}
        h_rows = np.zeros((npts, 32), np.uint8)
        h_status, h_best, h_med = (np.zeros(npts, np.int32) for _ in range(3))
        rows_flat, sig_flat, size_flat = (np.ascontiguousarray(W[k]) for k in ("rows", "sigma2", "size"))
        set_ptr = pt_ptr

        def host_route():
            host(W["cap"], 32, 32, 0, p_(rows_flat), p_(sig_flat), p_(size_flat), nk, p_(slots), p_(W["centres"]), p_(W["max_size"]), None, npts, p_(ids),
                 p_(W["ref"]), p_(pt_ptr), p_(W["obs_kf"]), p_(W["obs_idx"]), 0, 1, p_(h["pos"]), p_(h["normal"]), p_(h["min_distance"]),
                 p_(h["max_distance"]), p_(h["ref_size"]), p_(h["ref_distance"]), p_(h["ref_sigma"]), p_(flags), p_(h_rows), p_(h_status), p_(h_best), p_(h_med))
            via_host.set(ids, normal=h["normal"], min_distance=h["min_distance"], max_distance=h["max_distance"], ref_size=h["ref_size"],
                         ref_distance=h["ref_distance"], ref_sigma=h["ref_sigma"])
            chosen = None
            if descriptors:
                gathered = rows_flat[W["obs_kf"], W["obs_idx"]]        # every observed row out of its keyframe
                bi = np.zeros(npts, np.int32)
                bm = np.zeros(npts, np.int32)
                ctx.check(ctx.lib.afv_distinctive_descriptors(ctx.handle, p_(gathered), 32, p_(set_ptr), npts, p_(bi), p_(bm)), "afv_distinctive_descriptors")
                chosen = (pt_ptr[:-1] + bi).astype(np.int32)
                via_host.set_descriptors_from_table(ids, table, W["obs_kf"][chosen], W["obs_idx"][chosen])
            torch.cuda.synchronize()
            return chosen

        chosen = host_route()
        t_call, t_host = [], []
        for _ in range(a.calls):       # alternating: both routes meet the same neighbours on the machine
            t0 = time.perf_counter()
            call()
            t_call.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host_route()
            t_host.append(time.perf_counter() - t0)
        ga, gb = dev.get(ids), via_host.get(ids)
        same = all(ga[k].tobytes() == gb[k].tobytes() for k in ga) and bool(np.all(status == 0))
        if descriptors:
            same &= bool(np.array_equal(best, chosen))
        extra = dict(workload=label, points=npts, observations=ne, keyframes=nk, parts="both" if descriptors else "normals")
        stats("device: afv_table_refresh_points", t_call, equal_to_host_route=bool(same), **extra)
        stats("host route: tools/refresh_host.cpp%s + afv_points_set%s" % ((" + afv_distinctive_descriptors", " + _set_descriptors_from_table")
                                                                            if descriptors else ("", "")), t_host, **extra)
        for s in stores:
            s.close()
        table.close()
    tmp.cleanup()
    ctx.close()


if __name__ == "__main__":
    main()

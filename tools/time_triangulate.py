"""LocalMapping::CreateNewMapPoints on the device (afv_table_triangulate: two launches, the new points written into the resident store)
next to the same algorithm as a scalar host program (tools/triangulate_host.cpp, g++ -O3 -ffp-contract=off, compiled here) followed by
the afv_points_set / afv_points_set_descriptors upload the host route needs before SearchLocalPoints can see the points.  One current
keyframe and 20 neighbours of 1000 features each, about 150 matches per neighbour (SearchForTriangulation over a 50-node FeatureVector).
Host-to-host times over --calls calls each, median and spread, one JSON line per figure:

  the CreateNewMapPoints loop of DescriptorTable (per neighbour one match_triangulation and one triangulate call, masks updated between)
  the same loop in ONE call (CreateNewMapPointsChain: afv_table_create_new_points, the masks stay on the device between the neighbours);
    its observation list and masks are compared with the loop's once
  the match_triangulation calls of that loop alone
  ONE batched triangulate call over all 20 pairs (the matches of one batched match_triangulation call, masks of before the first neighbour)
  the host program fed those matches; the upload of its points

The batched call's answers are compared with the host program's, bit for bit.

    python tools/time_triangulate.py [--calls 200]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_triangulate.py --calls 20
(k_tri_points, k_tri_store, k_match_tri; k_newpts_judge, k_newpts_store)"""
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
FX, FY, CX, CY = 517.3, 516.5, 318.6, 255.3
N, NN, SHARED, NODES, CAP, TOL = 1000, 20, 190, 50, 1024, 1.2


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def twc(R, t):
    return np.array([-R[0, k] * t[0] + (-R[1, k] * t[1] + -R[2, k] * t[2]) for k in range(3)], f32)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def world(seed=1):
    """keyframe 0 sees N points; neighbour k sees SHARED of them (and N - SHARED points of its own), 0.5 px of noise, two flipped bits"""
    rs = np.random.RandomState(seed)
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    kfs = []
    pw = np.stack([rs.uniform(-2, 2, N), rs.uniform(-1.5, 1.5, N), rs.uniform(3, 9, N)], 1)
    base = rs.randint(0, 256, (N, 32)).astype(np.uint8)
    for k in range(NN + 1):
        a = 0.0 if k == 0 else rs.uniform(-0.08, 0.08)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Cc = np.zeros(3) if k == 0 else np.array([rs.choice([-1, 1]) * rs.uniform(0.3, 0.9), rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1)])
        R32, t32 = R.astype(f32), (-R @ Cc).astype(f32)
        if k == 0:
            src, P, D = np.arange(N), pw, base
        else:
            src = np.concatenate([rs.permutation(N)[:SHARED], -np.ones(N - SHARED, np.int64)])
            own = np.stack([rs.uniform(-2, 2, N), rs.uniform(-1.5, 1.5, N), rs.uniform(3, 9, N)], 1)
            P = np.where(src[:, None] >= 0, pw[np.clip(src, 0, None)], own)
            D = np.where(src[:, None] >= 0, base[np.clip(src, 0, None)], rs.randint(0, 256, (N, 32)).astype(np.uint8)).astype(np.uint8)
            D[np.arange(N), rs.randint(0, 32, N)] ^= (1 << rs.randint(0, 8, N)).astype(np.uint8)
            order = rs.permutation(N)
            src, P, D = src[order], P[order], D[order]
        pc = P @ R.T + t32.astype(np.float64)
        x = (FX * pc[:, 0] / pc[:, 2] + CX + rs.normal(0, 0.5, N)).astype(f32)
        y = (FY * pc[:, 1] / pc[:, 2] + CY + rs.normal(0, 0.5, N)).astype(f32)
        octave = rs.randint(0, 3, N)
        size = (f32(TOL) ** octave).astype(f32)
        node = np.where(src >= 0, src % NODES, rs.randint(0, NODES, N))      # a point falls into the same node in every keyframe
        order = np.argsort(node, kind="stable")
        seg_ptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=NODES))]).astype(np.int32)
        cam = {"Rcw": R32.reshape(9), "tcw": t32, "Ow": twc(R32, t32), "fx": f32(FX), "fy": f32(FY), "cx": f32(CX), "cy": f32(CY), "invfx": f32(1) / f32(FX),
               "invfy": f32(1) / f32(FY), "mb": f32(0.08), "mbf": f32(40.0), "ratio_factor": f32(1.5) * f32(TOL), "max_size": f32(TOL) ** 7}
        kfs.append(dict(x=x, y=y, sigma2=(size * size).astype(f32), size=size, desc=D, cam=cam, R=R, t=-R @ Cc, seg_ptr=seg_ptr, seg_idx=order.astype(np.int32)))
    F12, ep = [], []
    for k in range(1, NN + 1):
        R2, t2 = kfs[k]["R"], kfs[k]["t"]
        R12 = R2.T
        t12 = -R12 @ t2
        F12.append((np.linalg.inv(K).T @ skew(t12) @ R12 @ np.linalg.inv(K)).astype(f32).reshape(9))
        ep.append(np.array([FX * t2[0] / t2[2] + CX, FY * t2[1] / t2[2] + CY], f32))
    return kfs, np.stack(F12), np.stack(ep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_triangulate.py measures on the GPU: none found")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    so = os.path.join(tmp.name, "triangulate_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "triangulate_host.cpp"), "-o", so], check=True)
    host = C.CDLL(so).triangulate_host
    host.restype = C.c_int
    kfs, F12, ep = world()
    table = afv.table.DescriptorTable(ctx, NN + 1, CAP)
    points = afv.MapPoints(ctx, 8192)
    for k, kf in enumerate(kfs):
        table.set(k, kf["desc"])
        table.set_featvec(k, np.arange(NODES), kf["seg_ptr"], kf["seg_idx"])
        table.set_geometry(k, kf["x"], kf["y"], kf["sigma2"])
        table.set_scale(k, kf["size"])
    nbs = list(range(1, NN + 1))
    cams = {k: kf["cam"] for k, kf in enumerate(kfs)}
    fresh = lambda: {k: np.zeros(N, np.uint8) for k in range(NN + 1)}
    th = 50.0

    made = table.CreateNewMapPoints(points, 0, nbs, cams, F12, ep, th, fresh(), 0)
    t_loop, t_match = [], []
    for _ in range(a.calls):
        masks = fresh()
        t0 = time.perf_counter()
        table.CreateNewMapPoints(points, 0, nbs, cams, F12, ep, th, masks, 0)
        t_loop.append(time.perf_counter() - t0)
    loop_masks, chain_masks = fresh(), fresh()
    table.CreateNewMapPoints(points, 0, nbs, cams, F12, ep, th, loop_masks, 0)
    chained = table.CreateNewMapPointsChain(points, 0, nbs, cams, F12, ep, th, chain_masks, 0)
    chain_same = bool(chained == made and all(np.array_equal(loop_masks[k], chain_masks[k]) for k in loop_masks))
    t_chain = []
    for _ in range(a.calls):
        masks = fresh()
        t0 = time.perf_counter()
        table.CreateNewMapPointsChain(points, 0, nbs, cams, F12, ep, th, masks, 0)
        t_chain.append(time.perf_counter() - t0)
    # the call alone: records and cap-wide masks prepared outside the clock (what a C++ caller pays)
    chain_jobs = table.tri_points_jobs([cams[0]] * NN, [cams[nb] for nb in nbs], cams[0]["ratio_factor"], cams[0]["max_size"])
    t_call = []
    for _ in range(a.calls):
        m_cur, m_nb = np.zeros(CAP, np.uint8), np.zeros((NN, CAP), np.uint8)
        t0 = time.perf_counter()
        table.create_new_points(0, nbs, F12, ep, th, chain_jobs, m_cur, m_nb, points, 0)
        t_call.append(time.perf_counter() - t0)
    for _ in range(a.calls):
        masks = fresh()
        t0 = time.perf_counter()
        for k, nb in enumerate(nbs):
            table.match_triangulation([0], [nb], F12[k:k + 1], ep[k:k + 1], th, [masks[0]], [masks[nb]])
        t_match.append(time.perf_counter() - t0)

    masks = fresh()
    m12, nm = table.match_triangulation([0] * NN, nbs, F12, ep, th, [masks[0]] * NN, [masks[nb] for nb in nbs])
    jobs = table.tri_points_jobs([cams[0]] * NN, [cams[nb] for nb in nbs], cams[0]["ratio_factor"], cams[0]["max_size"])
    status, route, x3d, new_id, n_new = table.triangulate([0] * NN, nbs, jobs, m12, points, 0)
    t_batch = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        table.triangulate([0] * NN, nbs, jobs, m12, points, 0)
        t_batch.append(time.perf_counter() - t0)

    # the host route: the same matches through the scalar program, then the upload of what it made
    def planes(kf):
        p = np.zeros((8, CAP), f32)
        for r, key in enumerate(("x", "y", "sigma2")):
            p[r, :N] = kf[key]
        p[3], p[5] = -1.0, -1.0
        p[4, :N], p[6, :N], p[7, :N] = kf["size"], kf["x"], kf["y"]
        return p
    pa, pb = planes(kfs[0]), np.stack([planes(kfs[nb]) for nb in nbs])
    jf = np.zeros((NN, 47), f32)
    for p in range(NN):
        jf[p] = np.frombuffer(bytes(jobs[p])[4:], f32)
    mx = 8192
    h_status, h_route, h_x3d = np.zeros((NN, CAP), np.uint8), np.zeros((NN, CAP), np.uint8), np.zeros((NN, CAP, 3), f32)
    h_pos, h_nrm, h_f5, h_feat = np.zeros((mx, 3), f32), np.zeros((mx, 3), f32), np.zeros((5, mx), f32), np.zeros(mx, np.int32)
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)

    def run_host():
        return host(NN, CAP, N, p_(pa), p_(pb), p_(jf), p_(m12), p_(h_status), p_(h_route), p_(h_x3d), mx, p_(h_pos), p_(h_nrm), p_(h_f5), p_(h_feat))

    def upload(n):
        ids = np.arange(n, dtype=np.int32)
        points.set(ids, pos=h_pos[:n], normal=h_nrm[:n], min_distance=h_f5[0, :n], max_distance=h_f5[1, :n], ref_size=h_f5[2, :n], ref_distance=h_f5[3, :n],
                   ref_sigma=h_f5[4, :n])
        points.set_flags(ids, bad=np.zeros(n, np.uint8), observed=np.ones(n, np.uint8))
        points.set_descriptors_from_table(ids, table, np.zeros(n, np.int32), h_feat[:n])
        points.get(ids[:1])      # the setters are asynchronous: wait for them as the device route's call waits for its launches

    n_host = run_host()
    same = bool(n_host == int(n_new.sum()) and np.array_equal(h_status, status) and np.array_equal(h_route, route) and
                h_x3d.tobytes() == x3d.tobytes())
    t_host, t_up = [], []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        run_host()
        t_host.append(time.perf_counter() - t0)
    upload(n_host)
    for _ in range(a.calls):
        t0 = time.perf_counter()
        upload(n_host)
        t_up.append(time.perf_counter() - t0)
    extra = dict(neighbours=NN, features=N, matches_per_neighbour=float(np.mean(nm)))
    stats("device: CreateNewMapPoints loop, one neighbour at a time", t_loop, new_points=len(made), **extra)
    stats("device: the CreateNewMapPoints loop in one call (afv_table_create_new_points)", t_chain, new_points=len(chained), equal_to_the_loop=chain_same, **extra)
    stats("device: ... create_new_points alone, job records built beforehand", t_call)
    stats("device: the %d match_triangulation calls of that loop alone" % NN, t_match)
    stats("device: one batched afv_table_triangulate over %d pairs (store written)" % NN, t_batch, new_points=int(n_new.sum()), equal_to_host_program=same, **extra)
    stats("host program over the same matches", t_host, new_points=int(n_host))
    stats("host route: afv_points_set + set_flags + set_descriptors_from_table of its points", t_up, new_points=int(n_host))
    tmp.cleanup()
    points.close()
    table.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Global bundle adjustment on the device (afv_table_global_bundle_adjust: the block-sparse Schur solve of csrc/k_gba.hip, one wait per
trial) next to the same algorithm as a scalar host program (gba_host of tools/lba_host.cpp, g++ -O3 -ffp-contract=off: tools/
libgba_host.so, which python __graft_entry__.py builds).  Host-to-host times over --calls calls, median with [fastest, slowest]; the
device and the host program run ALTERNATING in one run and their answers are compared bit for bit in that run; write_points = 0, so
every call starts from the same store.  One JSON line per figure.

  chain maps (the call of LoopClosing::RunGlobalBundleAdjustment: 10 iterations, no kernel, no checks): keyframes on a closed path,
  keyframe i covisible with its 10 predecessors, one loop pair from the last keyframe to the first free one, about 100 points per
  keyframe, every point seen by four keyframes, keyframe 0 fixed: 300 and 1000 keyframes (--calls-large for the second)
  40 free + 40 fixed (the larger workload of tools/time_lba.py, LocalBundleAdjustment): the dense route (afv_table_bundle_adjust) and the
  sparse route on the same input in the same run, and the host program

Each line carries the blocks of L, the structural blocks among them and the fill.

    python tools/time_gba.py [--calls 200] [--calls-large 20] [--sizes 300,1000]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_gba.py --calls 3
--calls-large 3  (k_gba_*, k_lba_*; no counters in that run)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
f32 = np.float32
FX, FY, CX, CY, BF = 517.3, 516.5, 318.6, 255.3, 40.0
VIEWS, PER_KF, BAND = 4, 100, 10
NEW, OLD = "afv_table_global_bundle_adjust", "afv_table_bundle_adjust"


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def chain_world(n, seed=1):
    """n keyframes on a circle looking outward (position 0 is keyId 0: fixed, last in the list; position c >= 1 is list entry c - 1), a
    point anchored at position i is seen by i and three of its 10 predecessors; 8 points join the last position to position 1"""
    rs = np.random.RandomState(seed)
    r = 0.15 * n / (2 * np.pi)
    entry = lambda c: c - 1 if c >= 1 else n - 1
    cams = np.zeros((n, 17), np.float64)
    Rwc, Cw = {}, {}
    for c in range(n):
        th = 2 * np.pi * c / n
        Rwc[c] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        Cw[c] = r * np.array([np.sin(th), 0.0, np.cos(th)]) + [0.0, 0.01 * (c % 5), 0.0]
        k = entry(c)
        cams[k, :9], cams[k, 9:12] = Rwc[c].T.reshape(9), -Rwc[c].T @ Cw[c]
        cams[k, 12:17] = (FX, FY, CX, CY, BF)
    cams = cams.astype(f32)
    npts = n * PER_KF // VIEWS
    seen = []
    for p in range(npts):
        i = rs.randint(0, n)
        before = [c for c in range(i - BAND, i) if c >= 0]
        seen.append((i, sorted([i] + list(rs.choice(before, min(VIEWS - 1, len(before)), replace=False))) if before else [i]))
    seen += [(n - 1, [1, n - 1])] * 8
    npts = len(seen)
    feats = [dict(x=[], y=[], ur=[], inf=[]) for _ in range(n)]
    X = np.zeros((npts, 3))
    e_pt, e_kf, e_idx = [], [], []
    for p, (i, cs) in enumerate(seen):
        X[p] = Rwc[i] @ np.array([rs.uniform(-1.5, 1.5), rs.uniform(-1, 1), rs.uniform(4, 9)]) + Cw[i]
        for c in cs:
            k = entry(c)
            cam = cams[k].astype(np.float64)
            q = cam[:9].reshape(3, 3) @ X[p] + cam[9:12]
            f = feats[k]
            e_pt.append(p); e_kf.append(k); e_idx.append(len(f["x"]))
            f["x"].append(FX * q[0] / q[2] + CX + rs.normal(0, 0.5)); f["y"].append(FY * q[1] / q[2] + CY + rs.normal(0, 0.5))
            f["ur"].append(-1.0); f["inf"].append(1.0 / 1.2 ** (2 * rs.randint(0, 8)))
    start = cams.copy()
    start[:n - 1, 9:12] += rs.normal(0, 0.01, (n - 1, 3)).astype(f32)
    return dict(nk=n, nf=n - 1, np=npts, cams=start, pos=(X + rs.normal(0, 0.03, X.shape)).astype(f32),
                feats=[{m: np.asarray(v, f32) for m, v in f.items()} for f in feats],
                e_pt=np.asarray(e_pt, np.int32), e_kf=np.asarray(e_kf, np.int32), e_idx=np.asarray(e_idx, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--calls-large", type=int, default=0, help="calls of the 1000-keyframe map (0: as many as --calls)")
    ap.add_argument("--sizes", default="300,1000")
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_gba.py measures on the GPU: none found")
    lba = importlib.import_module("anyfeature-vslam_amd.lba")
    import time_lba
    so = os.path.join(ROOT, "tools", "libgba_host.so")
    if not os.path.exists(so):
        raise SystemExit("tools/libgba_host.so is missing: python __graft_entry__.py builds it")
    lib = C.CDLL(so)
    lib.gba_host.restype = C.c_int
    lib.lba_host.restype = None
    ctx = afv.Context()
    p_ = lambda v: v.ctypes.data_as(C.c_void_p)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    work = [("chain of %d keyframes" % n, chain_world(n), (10, 0), (0, 0), 0, (a.calls_large or a.calls) if n >= 1000 else a.calls, False) for n in sizes]
    work.append(("40 free + 40 fixed", time_lba.world(40, 40), (5, 10), (1, 0), 1, a.calls, True))
    all_equal = True
    for label, W, iters, robust, checks, calls, both in work:
        nk, nf, npts, ne = W["nk"], W["nf"], W["np"], len(W["e_pt"])
        cap = max(len(f["x"]) for f in W["feats"])
        table = afv.table.DescriptorTable(ctx, nk, cap)
        points = afv.MapPoints(ctx, npts)
        ids = np.arange(npts, dtype=np.int32)
        points.set(ids, pos=W["pos"])
        for k, f in enumerate(W["feats"]):
            m = len(f["x"])
            table.set(k, np.zeros((m, 32), np.uint8))
            table.set_geometry(k, f["x"], f["y"], np.ones(m, f32), u_right=f["ur"])
            table.set_inf(k, f["inf"])
        recs = lba.lba_cams([dict(Rcw=c[:9], tcw=c[9:12], fx=c[12], fy=c[13], cx=c[14], cy=c[15], mbf=c[16]) for c in W["cams"]])
        slots = np.arange(nk, dtype=np.int32)
        device = lambda entry: lba.bundle_adjust(table, points, slots, nf, recs, ids, W["e_pt"], W["e_kf"], W["e_idx"], iters, robust, checks,
                                                 write_points=False, entry=entry)
        obs = np.zeros((ne, 4), f32)
        for e in range(ne):
            f = W["feats"][W["e_kf"][e]]
            obs[e] = (f["x"][W["e_idx"][e]], f["y"][W["e_idx"][e]], f["ur"][W["e_idx"][e]], f["inf"][W["e_idx"][e]])
        params = np.array([iters[0], iters[1], robust[0], robust[1], checks, -1], np.int32)
        ok = np.ones(npts, np.uint8)
        ints, dbl, hkf, hxyz, hstate, extra = np.zeros(8, np.int32), np.zeros(4), np.zeros((nf, 12)), np.zeros((npts, 3)), np.zeros(ne, np.uint8), np.zeros(3, np.int32)
        cams_f, pos_f = np.ascontiguousarray(W["cams"]), np.ascontiguousarray(W["pos"])

        def host():
            return lib.gba_host(nk, nf, npts, ne, p_(cams_f), p_(pos_f), p_(ok), p_(W["e_pt"]), p_(W["e_kf"]), p_(obs), p_(params), C.c_longlong(1 << 20),
                                p_(ints), p_(dbl), p_(hkf), p_(hxyz), p_(hstate), p_(extra))

        def equal(out):
            res, kf, xyz, state = out
            same = [*res.iterations, *res.trials, res.n_edges, res.n_removed_first, res.n_erase, res.stopped] == list(ints)
            same &= np.array(list(res.chi2) + list(res.lam)).tobytes() == dbl.tobytes()
            return bool(same and kf.tobytes() == hkf.tobytes() and xyz.tobytes() == hxyz.tobytes() and np.array_equal(state, hstate))
        assert host() == 0
        out = device(NEW)
        same = equal(out)
        if both:
            same &= equal(device(OLD))
        all_equal &= same
        t = {NEW: [], OLD: [], "host": []}
        for _ in range(calls):                       # alternating: device, (dense device,) host program
            for entry in ([NEW, OLD] if both else [NEW]):
                t0 = time.perf_counter()
                device(entry)
                t[entry].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            host()
            t["host"].append(time.perf_counter() - t0)
        res = out[0]
        info = dict(free=nf, fixed=nk - nf, points=npts, edges=ne, iterations=sum(res.iterations), trials=sum(res.trials), calls=calls,
                    l_blocks=int(extra[0]), structural_blocks=int(extra[1]), fill_blocks=int(extra[0] - extra[1]), solve_fail=int(extra[2]),
                    all_blocks=nf * (nf + 1) // 2)
        stats(label + " | device: afv_table_global_bundle_adjust (block-sparse)", t[NEW], equal_to_host_program=same, **info)
        if both:
            stats(label + " | device: afv_table_bundle_adjust (dense)", t[OLD], **info)
        stats(label + " | host program: gba_host of tools/lba_host.cpp", t["host"], **info)
        points.close()
        table.close()
    ctx.close()
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())

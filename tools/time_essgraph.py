"""Times afv_essential_graph (the device) against tools/essgraph_host.cpp (one host core, the same arithmetic) on the same inputs in one
run, host to host, and checks that the two answers are bit-equal: medians of --calls calls [fastest, slowest].  The timed device calls correct
the points with write_points = 0 (xyz_out and the statuses come back, the store stays, so every call sees the same store); the host
route corrects a copy.  Two scenes: a chain of 200
keyframes with band 10 and one loop edge, and a chain of 1000 keyframes with 20000 points corrected.  The README's "Essential graph"
table is this tool's output; kernel times come from a rocprofv3 --kernel-trace --stats run of their own (python tools/time_essgraph.py
--calls 3 under the profiler).  python tools/time_essgraph.py [--calls N]"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--calls-large", type=int, default=0, help="calls of the 1000-keyframe scene (0: as many as --calls; a call takes most of a second on either route)")
    a = ap.parse_args()
    import _essgraph_host as H
    import _essgraph_scenes as SC
    afv = importlib.import_module("anyfeature-vslam_amd")
    so = os.path.join(ROOT, "tools", "libessgraph_host.so")
    if not os.path.exists(so):
        raise SystemExit("tools/libessgraph_host.so is missing: python __graft_entry__.py builds it")
    lib = C.CDLL(so)
    lib.essgraph_host.restype = None
    lib.essgraph_host_correct.restype = None
    ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    rows = []
    for label, n, band, npts in (("200 keyframes, band 10, one loop edge", 200, 10, 0), ("1000 keyframes, band 10, 20000 points", 1000, 10, 20000)):
        sc = SC.drifted(n, band, drift=0.002, edges=[(n - 1, 1)] + SC.band_edges(n, band, loop=False))
        pos, flags, ids, ref = SC.points_for(sc, n=npts, cap=max(npts, 1), seed=9) if npts else (np.zeros((1, 3), np.float32), np.zeros(1, np.uint8), None, None)
        pts = None
        if npts:
            pts = afv.MapPoints(ctx, len(pos))
            on = np.nonzero(flags & 1)[0].astype(np.int32)
            pts.set(on, pos=pos[on])
            pts.set_flags(on, bad=(flags[on] & 2) != 0)
        S, M = H.records(sc["S_init"]), H.records(sc["meas"])

        def device():
            return afv.essgraph.essential_graph(ctx, pts, S, sc["fixed"], sc["v0"], sc["v1"], M, sc["iterations"], 1e-16, sc["fix_scale"], ids, ref,
                                                write_points=False)

        def host():
            r = H.run_host(lib, sc)
            if npts:
                r.xyz, r.pst = H.host_correct(lib, pos.copy(), flags, ids, ref, S, r.Swc)
            return r

        dres, dS, dT, dx, dst = device()
        h = host()
        equal = (dS.tobytes() == h.S.tobytes() and dT.tobytes() == h.Tiw.tobytes() and (dres.iterations, dres.trials) == (h.iterations, h.trials) and
                 (not npts or (dx.tobytes() == h.xyz.tobytes() and np.array_equal(dst, h.pst))))

        def timed(fn, calls):
            t = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return np.median(t), min(t), max(t)
        calls = a.calls if n < 1000 else (a.calls_large or a.calls)
        td, th = timed(device, calls), timed(host, calls)
        rows.append((label + ", %d calls" % calls, dres.iterations, dres.trials, dres.l_blocks, td, th, equal))
        if pts is not None:
            pts.close()
    for label, it, tr, lb, td, th, equal in rows:
        print("%s: %d iterations, %d trials, %d blocks of L | device %.2f ms [%.2f, %.2f] | host program %.2f ms [%.2f, %.2f] | bit-equal: %s"
              % (label, it, tr, lb, td[0], td[1], td[2], th[0], th[1], th[2], equal))
    ctx.close()
    return 0 if all(r[-1] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())

"""Frame::ComputeStereoMatches on two resident frames (afv_frame_stereo_match) next to the path an integrator had before it: pull the 16
pyramid levels back (afv_debug_get_level), walk Frame.cc:465-645 on one core (tools/stereo_host_walk.cpp, compiled here with g++), upload
mvuRight again (afv_frame_set_features).  Two 640 x 480 frames of about 1000 features: the synthetic 'corners' frame and the same frame
moved a few pixels.  Host-to-host times; warm-up, then timed blocks: median and spread.  The two paths' mvuRight / mvDepth are compared
bit for bit.  One JSON line per path.

    python tools/time_stereo.py [--blocks 20] [--shift 6]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_stereo.py --blocks 1  (k_stereo_match,
k_stereo_median)"""
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
MBF, FX, TH = 40.0, 500.0, 75.0


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--shift", type=int, default=6)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_stereo.py measures on the GPU: none found")
    ptr = afv._lib.ptr
    ctx = afv.Context()
    img = afv.synth.corners_frame(1)
    imgs = (img, np.ascontiguousarray(np.roll(img, -a.shift, axis=1)))
    # ---- the device path: the frames keep their pyramids, the search runs where they lie ----
    left, right = afv.Frame(ctx, keep_pyramid=True), afv.Frame(ctx, keep_pyramid=True)
    (kl, dl), (kr, dr) = left.extract(imgs[0]), right.extract(imgs[1])
    n_dev = left.ComputeStereoMatches(right, MBF, FX, TH, TH)   # warm-up
    times = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        left.ComputeStereoMatches(right, MBF, FX, TH, TH)
        times.append(time.perf_counter() - t0)
    dev_ur, dev_dp = left.mvuRight.copy(), left.mvDepth.copy()
    stats("afv_frame_stereo_match (resident frames)", times, features=[len(kl), len(kr)], n_stereo=n_dev)
    # ---- the path of before: levels back to the host, the walk on one core, mvuRight up again ----
    plain_l, plain_r = afv.Frame(ctx), afv.Frame(ctx)
    g = ctx.geometry()
    nl = g["nlevels"]
    lw, lh = np.asarray(g["lw"][:nl], np.int32), np.asarray(g["lh"][:nl], np.int32)
    sl, sr = ctx.size_sigma(kl)[0], ctx.size_sigma(kr)[0]
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "stereo_host_walk.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "stereo_host_walk.cpp"), "-o", so],
                       check=True)
        walk = C.CDLL(so).stereo_host_walk
        walk.restype = C.c_int
        ur, dp = np.zeros(len(kl), np.float32), np.zeros(len(kl), np.float32)

        # timed pieces: 16 x afv_debug_get_level, the walk, afv_frame_set_features
        t_levels, t_walk, t_up = [], [], []
        for it in range(a.blocks + 1):
            lv = []
            dt = 0.0
            for fr, im in ((plain_l, imgs[0]), (plain_r, imgs[1])):
                fr.extract(im, host_outputs=False)
                t0 = time.perf_counter()
                lv.append([ctx.debug_level(0, l) for l in range(nl)])
                dt += time.perf_counter() - t0
            pl = (C.c_void_p * nl)(*[x.ctypes.data for x in lv[0]])
            pr = (C.c_void_p * nl)(*[x.ctypes.data for x in lv[1]])
            t0 = time.perf_counter()
            kept = walk(ptr(kl), ptr(sl), ptr(dl), len(kl), ptr(kr), ptr(sr), ptr(dr), len(kr), pl, pr, ptr(lw), ptr(lh), nl, C.c_float(MBF), C.c_float(FX),
                        C.c_float(TH), C.c_float(TH), ptr(ur), ptr(dp))
            t1 = time.perf_counter()
            plain_l.set_features(kl, dl, sizes=sl, u_right=ur)
            t2 = time.perf_counter()
            if it:  # the first round warms up
                t_levels.append(dt); t_walk.append(t1 - t0); t_up.append(t2 - t1)
        total = [x + y + z for x, y, z in zip(t_levels, t_walk, t_up)]
        same = ur.tobytes() == dev_ur.tobytes() and dp.tobytes() == dev_dp.tobytes() and kept == n_dev
        stats("16 x afv_debug_get_level + host walk + afv_frame_set_features", total, levels_ms_median=1e3 * sorted(t_levels)[len(t_levels) // 2],
              walk_ms_median=1e3 * sorted(t_walk)[len(t_walk) // 2], upload_ms_median=1e3 * sorted(t_up)[len(t_up) // 2], n_stereo=int(kept),
              equal_device_bits=bool(same))
    for fr in (left, right, plain_l, plain_r):
        fr.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Brute-force pair matching on a FLOAT keyframe table (config #4 shape): 1000 keyframes x 1000 rows, 10 000 LCG pair jobs through
DescriptorTable.match_pairs_device at 64 / 128 / 256 floats, rotation histogram off and on.  The rows are the config #4 recipe
(keyframe k+1 = keyframe k with every bit flipped w.p. 0.1 and 30 % of its rows replaced) turned into floats with full mantissas.
Yardstick at 64 and 128: afv_match_l2_pairs_device on the SAME device rows (the table's own d_desc), timed in the same run, the two
alternating block by block.  Warm-up, then timed blocks: median and spread of jobs/s.  One JSON line per (dim, path).

    python tools/time_table_float.py [--dims 64,128,256] [--blocks 5] [--reps 1]

Kernel times: run it again under  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_table_float.py --blocks 1 --reps 1"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def floaten(d32, dim):
    """the first `dim` bits of 32-byte rows scaled, plus a deterministic fraction per element: distances with full float mantissas"""
    bits = np.unpackbits(np.ascontiguousarray(d32, np.uint8), axis=1)[:, :dim].astype(np.float32)
    n = len(bits)
    frac = ((np.arange(n * dim, dtype=np.uint64).reshape(n, dim) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 20)).astype(np.float32)
    return np.ascontiguousarray(bits * np.float32(0.75) + frac * np.float32(0.2 / (1 << 20)), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1, help="calls of --jobs jobs per timed block")
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--jobs", type=int, default=10000)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    tbl = importlib.import_module("anyfeature-vslam_amd.table")
    dist = importlib.import_module("anyfeature-vslam_amd.dist")
    if not torch.cuda.is_available():
        sys.exit("time_table_float.py measures on the GPU: none found")
    K, cap, njobs = a.keyframes, 1000, a.jobs
    ctx = afv.Context()
    pa, pb = dist.lcg_pairs(12345, njobs, K)
    d_a, d_b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    t32, ang, cnt = afv.synth.keyframe_table(K, cap, nbytes=32)
    match = torch.empty((njobs, cap), dtype=torch.int32, device="cuda")
    nm = torch.empty((njobs,), dtype=torch.int32, device="cuda")
    for dim in [int(x) for x in a.dims.split(",")]:
        th = 75.0 * dim / 256.0 * 0.6
        table = tbl.DescriptorTable(ctx, K, cap, float_dim=dim)
        host = np.empty((K, cap, dim), np.float32)
        for k in range(K):
            host[k] = floaten(t32[k], dim)
        table.upload(host, ang, cnt)
        del host
        d_desc, _, d_n = table.device_views()
        raw = afv.FeatureMatcher(0.75, False, ctx=ctx)
        paths = [("table", lambda: table.match_pairs_device(d_a, d_b, th, 0.75, False, match, nm)),
                 ("table+orientation", lambda: table.match_pairs_device(d_a, d_b, th, 0.75, True, match, nm))]
        if dim in (64, 128):
            paths.insert(0, ("afv_match_l2_pairs_device", lambda: raw.match_l2_pairs_device(d_desc, d_n, d_a, d_b, th, 0.75, match, nm)))
        rates = {name: [] for name, _ in paths}
        means = {}
        for name, call in paths:  # warm-up
            call()
            torch.cuda.synchronize()
            means[name] = float(nm.float().mean().item())
        for _ in range(a.blocks):  # the paths alternate inside every block
            for name, call in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call()
                torch.cuda.synchronize()
                rates[name].append(a.reps * njobs / (time.perf_counter() - t0))
        for name, _ in paths:
            r = sorted(rates[name])
            print(json.dumps({"dim": dim, "path": name, "jobs_per_s_median": r[len(r) // 2], "jobs_per_s_min": r[0], "jobs_per_s_max": r[-1],
                              "mean_matches": means[name]}), flush=True)
        table.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Brute-force pair matching at several descriptor widths (config #4 shape): 1000 keyframes x 1000 rows, 10 000 LCG pair jobs through
DescriptorTable.match_pairs_device, the table built with the config #4 recipe at each width (keyframe k+1 = keyframe k with every bit
flipped w.p. 0.1 and 30 % of its rows replaced).  Both phase-1 engines; warm-up, then five timed blocks: median and spread of jobs/s.
One JSON line per (width, engine).

    python tools/time_table_widths.py [--widths 32,48,61,64] [--blocks 5] [--reps 3]

Kernel times: run it again under  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_table_widths.py --blocks 1 --reps 1"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _th(w):
    return {61: 128.0, 48: 120.0}.get(w, float(round(75.0 * w / 32.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="32,48,61,64")
    ap.add_argument("--engines", default="1,0")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls of 10 000 jobs per timed block")
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--jobs", type=int, default=10000)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    tbl = importlib.import_module("anyfeature-vslam_amd.table")
    dist = importlib.import_module("anyfeature-vslam_amd.dist")
    K, cap, njobs = a.keyframes, 1000, a.jobs
    ctx = afv.Context()
    pa, pb = dist.lcg_pairs(12345, njobs, K)
    d_a, d_b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    for w in [int(x) for x in a.widths.split(",")]:
        host = afv.synth.keyframe_table(K, cap, nbytes=w)
        table = tbl.DescriptorTable(ctx, K, cap, desc_bytes=w)
        table.upload(*host)
        match = torch.empty((njobs, cap), dtype=torch.int32, device="cuda")
        nm = torch.empty((njobs,), dtype=torch.int32, device="cuda")
        for eng in [int(x) for x in a.engines.split(",")]:
            ctx.set_match_engine(eng)
            for _ in range(2):  # warm-up
                table.match_pairs_device(d_a, d_b, _th(w), 0.75, True, match, nm)
            torch.cuda.synchronize()
            rates = []
            for _ in range(a.blocks):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    table.match_pairs_device(d_a, d_b, _th(w), 0.75, True, match, nm)
                torch.cuda.synchronize()
                rates.append(a.reps * njobs / (time.perf_counter() - t0))
            rates.sort()
            print(json.dumps({"width": w, "pitch": table.pitch, "engine": "mfma" if eng == 1 else "popcount", "jobs_per_s_median": rates[len(rates) // 2],
                              "jobs_per_s_min": rates[0], "jobs_per_s_max": rates[-1], "mean_matches": float(nm.float().mean().item())}), flush=True)
        ctx.set_match_engine(1)
        table.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Words in common + Vocabulary::score on the keyframe table (afv_table_score_bow): 1000 keyframes, 1000 features each, word ids of a
k = 10, L = 6 vocabulary (10^6 words); consecutive keyframes keep about 70 % of their words (the config #4 recipe).  Host-to-host time of
the 1 x 1000 call (one query slot, every slot) and of the 1000 x 1000 batch (ONE launch), next to the host walk an integrator had before:
DBoW2's L1 score over std::map BowVectors on one core (tools/bow_host_walk.cpp, compiled here with g++).  The scores of both paths are
compared bit for bit.  Warm-up, then timed blocks: median and spread.  One JSON line per path.

    python tools/time_table_bow.py [--blocks 5] [--keyframes 1000] [--host-queries 50]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_table_bow.py --blocks 1  (k_score_bow)"""
import argparse
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
NWORDS = 10 ** 6


def bow_vectors(K, nfeat, seed=7):
    """[(word int32[] ascending, value float64[] L1-normalised)]: keyframe k + 1 keeps ~70 % of keyframe k's words"""
    rng = np.random.RandomState(seed)
    words = rng.choice(NWORDS, nfeat, replace=False)
    out = []
    for _ in range(K):
        w = np.unique(words).astype(np.int32)
        v = 0.5 + rng.rand(len(w))
        out.append((w, v / v.sum()))
        fresh = rng.rand(nfeat) < 0.3
        words = np.where(fresh, rng.randint(0, NWORDS, nfeat), words)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--host-queries", type=int, default=50, help="queries the one-core host walk scores (its time is scaled to the batch)")
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_table_bow.py measures on the GPU: none found")
    K = a.keyframes
    bows = bow_vectors(K, a.features)
    ctx = afv.Context()
    table = afv.table.DescriptorTable(ctx, K, 1024)
    one = np.zeros((1, 32), np.uint8)
    for k, (w, v) in enumerate(bows):
        table.set(k, one)                       # a slot is scored when it holds features
        table.set_bowvec(k, w, v)
    paths = [("score_bow 1 x %d" % K, [0], 1), ("score_bow %d x %d" % (K, K), list(range(K)), K)]
    results = {}
    for name, queries, nq in paths:
        results[name] = table.score_bow(queries)          # warm-up (grows the staging buffers)
        times = []
        for _ in range(a.blocks):
            t0 = time.perf_counter()
            table.score_bow(queries)
            times.append(time.perf_counter() - t0)
        times.sort()
        print(json.dumps({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1],
                          "pairs_per_s_median": nq * K / times[len(times) // 2], "mean_common": float(results[name][0].mean())}), flush=True)
    # the host walk
    hq = min(a.host_queries, K)
    with tempfile.TemporaryDirectory() as tmp:
        exe, blob, out = os.path.join(tmp, "bow_host_walk"), os.path.join(tmp, "bows.bin"), os.path.join(tmp, "scores.bin")
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "bow_host_walk.cpp"), "-o", exe], check=True)
        with open(blob, "wb") as fh:
            fh.write(np.int32(K).tobytes())
            for w, v in bows:
                fh.write(np.int32(len(w)).tobytes() + w.tobytes() + np.ascontiguousarray(v, np.float64).tobytes())
        for name, nq in (("host std::map walk 1 x %d" % K, 1), ("host std::map walk %d x %d" % (hq, K), hq)):
            times = []
            for _ in range(max(a.blocks, 1)):
                times.append(float(subprocess.run([exe, blob, str(nq), out], check=True, capture_output=True, text=True).stdout))
            times.sort()
            host = np.fromfile(out, np.float64).reshape(nq, K)
            same = host.tobytes() == results[paths[1][0]][1][:nq].tobytes()
            print(json.dumps({"path": name, "ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1],
                              "pairs_per_s_median": nq * K / times[len(times) // 2], "scaled_to_%d_queries_ms" % K: 1e3 * times[len(times) // 2] * K / nq,
                              "scores_equal_device_bits": bool(same)}), flush=True)
    table.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Time Vocabulary.create (afv_vocab_train_device) on the reference's training shape with LCG descriptors: 10 842 images x 1000 x 32 B
(createVocabulary.cpp:122-179), k = 10 / L = 6 and k = 9 / L = 3 (createVocabulary.cpp:50-51).  Reports seconds in total and per level,
rounds per level and rows associated per second (rows of a level's non-trivial nodes x the level's rounds: an upper bound of the rows the
association kernel read, converged nodes drop out earlier); the median of --runs runs after one warm-up.  --ref-rows N also times the
plain-Python restatement (tests/_voctrain_ref.py) on the first N rows, for scale.  No threshold: nothing earlier exists to compare with.

    python tools/time_vocab_train.py [--images 10842] [--per-image 1000] [--runs 5] [--max-iters 0] [--ref-rows 100000] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10842)
    ap.add_argument("--per-image", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=0)
    ap.add_argument("--ref-rows", type=int, default=0)
    ap.add_argument("--shapes", default="10x6,9x3")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    ctx = afv.Context()
    n = a.images * a.per_image
    step = 1 << 20   # the LCG stream in pieces of 2^20 rows, a seed each (the jump tables of one 347 MB stream would take gigabytes)
    rows = np.concatenate([afv.synth.lcg_bytes(12345 + i, min(step, n - i) * 32).reshape(-1, 32) for i in range(0, n, step)])
    iptr = (np.arange(a.images + 1, dtype=np.int64) * a.per_image).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    result = {"images": a.images, "per_image": a.per_image, "rows": n, "desc_bytes": 32, "max_iters": a.max_iters, "runs": a.runs, "shapes": {}}
    for shape in a.shapes.split(","):
        k, L = [int(v) for v in shape.split("x")]
        totals, levels, rounds, work = [], [], None, None
        for run in range(a.runs + 1):   # the first run is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = afv.Vocabulary.create(dev, k, L, 0, ctx, a.max_iters, image_ptr=iptr, pitch=32)
            dt = time.perf_counter() - t0
            st = v.train_stats
            if run:
                totals.append(dt); levels.append(st["seconds"].tolist())
            rounds, work, words, capped = st["rounds"].tolist(), st["rows"].tolist(), v.size(), st["capped"]
            v.close()
        per_level = [statistics.median(l[i] for l in levels) for i in range(L)]
        assoc = sum(r * w for r, w in zip(rounds, work))
        result["shapes"][shape] = {"seconds_total_median": statistics.median(totals), "seconds_total_all": totals, "seconds_per_level": per_level,
                                   "rounds_per_level": rounds, "rows_per_level": work, "words": words, "capped": capped,
                                   "rows_associated": assoc, "rows_associated_per_second": assoc / max(sum(per_level), 1e-9)}
        print(shape, json.dumps(result["shapes"][shape]), flush=True)
    if a.ref_rows:
        import _voctrain_ref as R
        m = min(a.ref_rows, n)
        imgs = [rows[i:i + a.per_image] for i in range(0, m, a.per_image)]
        t0 = time.perf_counter()
        out = R.train(imgs, 32, 9, 3, 0, a.max_iters)
        result["restatement"] = {"rows": m, "k": 9, "L": 3, "seconds": time.perf_counter() - t0, "rounds_per_level": out["rounds"]}
        print("restatement", json.dumps(result["restatement"]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()

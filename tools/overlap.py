#!/usr/bin/env python3
"""Who runs beside whom?  Sibling of tools/timeline.py: runs bench.py under rocprofv3 --kernel-trace (nothing else traced) and prints, per
kernel name and per step of the timed region, the time its launches spend
  same   beside another launch of the SAME name (the two streams in lockstep: a heavy kernel beside its twin),
  other  beside launches of DIFFERENT names only (what the two-stream split is for),
  alone  with nothing beside them.
same + other + alone = the summed duration of the kernel's launches.
Usage: python tools/overlap.py [--root TREE] [--tag NAME] [--csv TRACE.csv] [--out DIR] [bench args]   -> DIR/NAME.json
  --out    where the trace and the summary go (default: overlap_out/ in this tree)
  --root   the tree whose bench.py runs (default: this one; a checkout of the parent commit for the before / after pair)
  --csv    analyse an existing kernel trace instead of running anything (steps = 6, warm-up = 2, as this tool records them)"""
import collections
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 6, 2


def load(path):
    rows = list(csv.DictReader(open(path)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "").split("<")[0]) for r in rows)
    return [e for e in ev if e[2].startswith("k_")]


def classify(ev):
    """ev: (start, end, name) in ns -> {name: [launches, same, other, alone]} (ns, summed over the launches)"""
    pts = sorted([(s, 1, n) for s, e, n in ev] + [(e, 0, n) for s, e, n in ev])  # at equal times the ends come first
    active = collections.Counter()
    res = {}
    last = pts[0][0] if pts else 0
    for t, start, n in pts:
        dur = t - last
        if dur > 0:
            depth = sum(active.values())
            for a, cnt in active.items():
                if not cnt:
                    continue
                r = res.setdefault(a, [0, 0, 0, 0])
                if cnt >= 2:
                    r[1] += dur * cnt
                elif depth > cnt:
                    r[2] += dur
                else:
                    r[3] += dur
        if start:
            active[n] += 1
            res.setdefault(n, [0, 0, 0, 0])[0] += 1
        else:
            active[n] -= 1
        last = t
    return res


def summarise(ev, steps):
    t0, t1 = ev[0][0], max(e[1] for e in ev)
    out = {"steps": steps, "wall_ms_per_step": (t1 - t0) / 1e6 / steps, "kernels": {}}
    for n, (cnt, same, other, alone) in sorted(classify(ev).items()):
        tot = same + other + alone
        out["kernels"][n] = {"launches_per_step": cnt / steps, "sum_ms_per_step": tot / 1e6 / steps, "same_ms_per_step": same / 1e6 / steps,
                             "other_ms_per_step": other / 1e6 / steps, "alone_ms_per_step": alone / 1e6 / steps,
                             "same_frac": same / tot if tot else 0.0}
    return out


def main():
    argv = sys.argv[1:]
    opt = {"--root": ROOT, "--tag": "overlap", "--csv": None, "--out": os.path.join(ROOT, "overlap_out")}
    while argv and argv[0] in opt:
        opt[argv[0]] = argv[1]
        argv = argv[2:]
    out = os.path.abspath(opt["--out"])
    os.makedirs(out, exist_ok=True)
    trace = opt["--csv"]
    if not trace:
        tdir = os.path.join(out, opt["--tag"] + "_trace")
        cmd = ["rocprofv3", "--kernel-trace", "-d", tdir, "-o", "ov", "--output-format", "csv", "--", sys.executable,
               os.path.join(os.path.abspath(opt["--root"]), "bench.py"), "--steps", str(STEPS), "--warmup", str(WARMUP), "--cpu-frames", "0", "--no-profile",
               "--no-extras"] + argv
        r = subprocess.run(cmd, env=dict(os.environ, TMPDIR="/tmp"), cwd="/tmp", stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
        found = glob.glob(os.path.join(tdir, "**", "ov_kernel_trace.csv"), recursive=True)
        if r.returncode or not found:
            sys.exit("overlap.py: the traced run failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]))
        trace = found[0]
    ev = load(trace)
    per_step = len(ev) // (STEPS + WARMUP)  # every step launches the same kernels
    res = summarise(ev[-per_step * STEPS:], STEPS)
    res["bench_args"] = argv
    json.dump(res, open(os.path.join(out, opt["--tag"] + ".json"), "w"), indent=1)
    print("%-28s %9s %9s %9s %9s %9s   (ms per step; wall %.3f)" % ("kernel", "launches", "sum", "same", "other", "alone", res["wall_ms_per_step"]))
    for n, k in res["kernels"].items():
        print("%-28s %9.1f %9.3f %9.3f %9.3f %9.3f" % (n, k["launches_per_step"], k["sum_ms_per_step"], k["same_ms_per_step"], k["other_ms_per_step"],
                                                       k["alone_ms_per_step"]))


if __name__ == "__main__":
    main()

"""Optimizer::PoseOptimization on the device (afv_frame_pose_optimize: one launch, everything it reads already resident) next to the
same algorithm as a scalar host program (tools/pose_opt_host.cpp, g++ -O3 -ffp-contract=off, compiled here): 1000 and 2000 edges on a
640 x 480 frame, 10 % planted outliers, 0.7 px of noise, the initial pose a perturbed true one.  Host-to-host times over --calls calls
each, median and spread.  The host program is built twice: with the binary-tree sums of the device (its answers are compared with the
device's, bit for bit) and with sums in feature order, as g2o runs them - the faster one is the baseline.  Then the chain
SearchLocalPoints -> PoseOptimization -> SearchLocalPoints on an extracted frame: with the optimisation on the device, and with the
matches copied out, the host program run and the pose handed back with set_pose.  One JSON line per figure.

    python tools/time_pose_opt.py [--calls 300]

Kernel time: run it again under  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_pose_opt.py --calls 20  (k_pose_optimize)"""
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
FX, FY, CX, CY, MBF = 517.3, 516.5, 318.6, 255.3, 40.0
W, H = 640.0, 480.0


def stats(name, times, **extra):
    times = sorted(times)
    print(json.dumps(dict({"path": name, "host_to_host_ms_median": 1e3 * times[len(times) // 2], "ms_min": 1e3 * times[0], "ms_max": 1e3 * times[-1]},
                          **extra)), flush=True)


def rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def twc(Rcw, tcw):
    return np.array([-Rcw[0, k] * tcw[0] + (-Rcw[1, k] * tcw[1] + -Rcw[2, k] * tcw[2]) for k in range(3)], f32)


def scene(n, seed):
    """n features, every one an edge: observations of points seen from a true pose, 10 % of them moved by 50 px"""
    rs = np.random.RandomState(seed)
    Rt, tt = rot(rs.normal(0, 0.2, 3)), rs.normal(0, 0.5, 3)
    u, v, z = rs.uniform(10, W - 10, n), rs.uniform(10, H - 10, n), rs.uniform(2.0, 10.0, n)
    pc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
    pw = ((pc - tt) @ Rt).astype(f32)
    pc = pw.astype(np.float64) @ Rt.T + tt
    x = FX * pc[:, 0] / pc[:, 2] + CX + rs.normal(0, 0.7, n)
    y = FY * pc[:, 1] / pc[:, 2] + CY + rs.normal(0, 0.7, n)
    ur = np.where(rs.rand(n) < 0.5, x - MBF / pc[:, 2] + rs.normal(0, 0.7, n), -1.0)
    planted = rs.rand(n) < 0.1
    ang = rs.uniform(0, 2 * np.pi, n)
    x, y = np.where(planted, x + 50 * np.cos(ang), x), np.where(planted, y + 50 * np.sin(ang), y)
    R0 = (rot(rs.normal(0, 0.02, 3)) @ Rt).astype(f32)
    t0 = (tt + rs.normal(0, 0.05, 3)).astype(f32)
    return dict(x=x.astype(f32), y=y.astype(f32), ur=ur.astype(f32), octave=rs.randint(0, 8, n).astype(np.int32), pos=pw, planted=planted, R0=R0, t0=t0,
                ids=rs.permutation(4096)[:n].astype(np.int32))


class HostProgram:
    def __init__(self, so):
        self.fn = C.CDLL(so).pose_opt_host
        self.fn.restype = C.c_int

    def __call__(self, x, y, ur, inf, pts, store_pos, store_set, cam, pose):
        n = len(x)
        out, outl, ints, dbl = np.zeros(12, f32), np.zeros(max(n, 1), np.uint8), np.zeros(10, np.int32), np.zeros(8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        ng = self.fn(n, p(x), p(y), p(ur), p(inf), p(pts), p(store_pos), p(store_set), len(store_set), p(cam), p(pose), p(out), p(outl), p(ints), p(dbl))
        return ng, out, outl[:n], ints, dbl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    import torch
    afv = importlib.import_module("anyfeature-vslam_amd")
    if not torch.cuda.is_available():
        sys.exit("time_pose_opt.py measures on the GPU: none found")
    ctx = afv.Context()
    tmp = tempfile.TemporaryDirectory()
    progs = {}
    for tag, flags in (("tree", ["-DPO_TREE"]), ("ordered", [])):
        so = os.path.join(tmp.name, "pose_opt_host_%s.so" % tag)
        subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"] + flags + [os.path.join(ROOT, "tools", "pose_opt_host.cpp"), "-o", so],
                       check=True)
        progs[tag] = HostProgram(so)
    cam = np.array([FX, FY, CX, CY, MBF], f32)
    for n in (1000, 2000):
        s = scene(n, n)
        points = afv.MapPoints(ctx, 4096)
        points.set(s["ids"], pos=s["pos"])
        frame = afv.Frame(ctx, max_x=W, max_y=H, cap=n)
        kps = np.zeros(n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = s["x"], s["y"], s["octave"]
        frame.set_features(kps, np.zeros((n, 32), np.uint8), u_right=s["ur"])
        frame.set_pose(s["R0"], s["t0"], twc(s["R0"], s["t0"]), *cam)
        inf = ctx.size_sigma(kps)[2]
        store_pos, store_set = np.zeros((4096, 3), f32), np.zeros(4096, np.uint8)
        store_pos[s["ids"]], store_set[s["ids"]] = s["pos"], 1
        pose = np.concatenate([s["R0"].reshape(9), s["t0"]]).astype(f32)
        dev = frame.PoseOptimizationBatch(points, [s["ids"]])[0]
        ng, out, outl, ints, dbl = progs["tree"](s["x"], s["y"], s["ur"], inf, s["ids"], store_pos, store_set, cam, pose)
        same = bool(ng == dev["n_good"] and out[:9].tobytes() == dev["Rcw"].tobytes() and out[9:].tobytes() == dev["tcw"].tobytes() and
                    np.array_equal(outl != 0, dev["outlier"]) and np.array_equal(ints[6:], dev["trials"]) and dbl[:4].tobytes() == dev["chi2"].tobytes())
        td, tt_, to = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            frame.PoseOptimizationBatch(points, [s["ids"]])
            td.append(time.perf_counter() - t0)
        for tag, acc in (("tree", tt_), ("ordered", to)):
            for _ in range(a.calls):
                t0 = time.perf_counter()
                progs[tag](s["x"], s["y"], s["ur"], inf, s["ids"], store_pos, store_set, cam, pose)
                acc.append(time.perf_counter() - t0)
        ngo = progs["ordered"](s["x"], s["y"], s["ur"], inf, s["ids"], store_pos, store_set, cam, pose)[0]
        extra = dict(edges=n, n_good=int(dev["n_good"]), planted=int(s["planted"].sum()), iterations=dev["iterations"].tolist(), trials=dev["trials"].tolist())
        stats("device: afv_frame_pose_optimize, %d edges" % n, td, equal_to_host_tree_program=same, **extra)
        stats("host program, tree sums, %d edges" % n, tt_, n_good=int(ng))
        stats("host program, ordered sums, %d edges" % n, to, n_good=int(ngo))
        frame.close()
        points.close()

    # the chain on an extracted frame: map points made from its keypoints at random depths, seen from the identity pose; the tracker starts
    # from a perturbed pose
    frame = afv.Frame(ctx)
    kps, desc = frame.extract(afv.synth.corners_frame(1))
    n = len(kps)
    rs = np.random.RandomState(7)
    z = rs.uniform(2.0, 10.0, n).astype(f32)
    pos = np.stack([(kps["x"] - CX) / FX * z, (kps["y"] - CY) / FY * z, z], 1).astype(f32)
    dist = np.linalg.norm(pos, axis=1).astype(f32)
    ids = rs.permutation(4096)[:n].astype(np.int32)
    points = afv.MapPoints(ctx, 4096)
    sizes, _, inf = ctx.size_sigma(kps)
    points.set(ids, pos=pos, normal=(pos / dist[:, None]).astype(f32), min_distance=dist * f32(0.7), max_distance=dist * f32(1.3), ref_size=sizes,
               ref_distance=dist, ref_sigma=np.full(n, 0.5, f32))
    points.set_flags(ids, bad=np.zeros(n), observed=np.ones(n))
    points.set_descriptors(ids, desc)
    store_pos, store_set = np.zeros((4096, 3), f32), np.zeros(4096, np.uint8)
    store_pos[ids], store_set[ids] = pos, 1
    R0 = rot(np.array([0.004, -0.003, 0.002])).astype(f32)
    t0 = np.array([0.01, -0.008, 0.012], f32)
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    m = afv.FeatureMatcher(0.8, False, ctx=ctx)
    ur = np.full(n, -1.0, f32)   # an extracted monocular frame: mvuRight = -1
    x, y = np.ascontiguousarray(kps["x"]), np.ascontiguousarray(kps["y"])

    def chain(on_device):
        frame.set_pose(R0, t0, twc(R0, t0), *cam)
        t_0 = time.perf_counter()
        a1, n1, _ = frame.SearchLocalPoints(m, points, ids, 3.0)
        pts = np.where(a1 >= 0, ids[np.clip(a1, 0, None)], -1).astype(np.int32)
        if on_device:
            ng, outl, Tcw = frame.PoseOptimization(points, pts)
            Rn, tn = Tcw[:3, :3], Tcw[:3, 3]
        else:
            ng, out, outl, _, _ = progs["ordered"](x, y, ur, inf, pts, store_pos, store_set, cam, np.concatenate([R0.reshape(9), t0]).astype(f32))
            Rn, tn = out[:9].reshape(3, 3), out[9:]
            frame.set_pose(Rn, tn, twc(Rn, tn), *cam)
        a2, n2, _ = frame.SearchLocalPoints(m, points, ids, 3.0)
        return time.perf_counter() - t_0, n1, int(ng), n2

    for on_device, name in ((True, "chain search -> optimise on the device -> search"), (False, "chain search -> host program + set_pose -> search")):
        chain(on_device)
        res = [chain(on_device) for _ in range(a.calls)]
        stats(name, [r[0] for r in res], features=n, matches_before=res[0][1], n_good=res[0][2], matches_after=res[0][3])
    tmp.cleanup()
    points.close()
    frame.close()
    ctx.close()


if __name__ == "__main__":
    main()

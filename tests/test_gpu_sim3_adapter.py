"""-m gpu: afv::Sim3Solver of adapter/afv_adapter.hpp as a plain C++ process (adapter/sim3_selftest): a seeded world of a current keyframe
and three candidates goes in as a file, the trace of LoopClosing's iterate(5) loop comes out and is held to the trace the Python class
(Sim3Solver.batch) computes on the same world."""
import os
import subprocess

import numpy as np
import pytest

import _sim3_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "sim3_selftest")
CAP, N, NHYP, MIN_INLIERS, MAX_ITS, SEED = 64, 30, 48, 12, 48, 12345


def _hx(v):
    return float(np.float32(v)).hex()


def _cam(c):
    return " ".join(_hx(v) for v in list(c.Rcw) + list(c.tcw) + [c.fx, c.fy, c.cx, c.cy])


def test_cpp_adapter_iterates_as_the_python_class(afv, gpu_ctx, tmp_path):
    assert os.path.exists(BIN), "sim3_selftest is not built: __graft_entry__.build() compiles it"
    cands = [S.world(70, n=N, s=0.5, outliers=o, noise=0.3) for o in (0.2, 0.5, 0.9)]    # one seed: the same keyframe 1 and map 1
    base, nc, n2 = cands[0], len(cands), cands[0].n2
    # one store: ids 0 .. N - 1 map 1 (the same for every candidate), then N ids of map 2 per candidate; one point of map 1 is bad
    pos = np.concatenate([base.pos[:N]] + [sc.pos[N:] for sc in cands])
    bad = np.zeros(len(pos), np.uint8)
    bad[4] = 1
    mp1 = np.arange(N, dtype=np.int32)
    mp2 = np.stack([N * (c + 1) + np.arange(N, dtype=np.int32) for c in range(nc)])
    mp2[1, 7] = -1
    idx2 = np.stack([sc.idx2 for sc in cands])
    lines = ["%d %d %d %d %d 0 %d %d %d %d" % (CAP, nc, N, n2, len(pos), SEED, NHYP, MIN_INLIERS, MAX_ITS), _cam(base.cam1)]
    lines += ["%s %d" % (_hx(base.sigma2_1[i]), mp1[i]) for i in range(N)]
    for c, sc in enumerate(cands):
        lines.append(_cam(sc.cam2))
        lines.append(" ".join(_hx(v) for v in sc.sigma2_2))
        lines += ["%d %d" % (mp2[c, i], idx2[c, i]) for i in range(N)]
    lines += ["%s %s %s %d" % (_hx(p[0]), _hx(p[1]), _hx(p[2]), b) for p, b in zip(pos, bad)]
    inp = tmp_path / "world.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the same world through the Python class
    table = afv.table.DescriptorTable(gpu_ctx, nc + 1, CAP)
    points = afv.MapPoints(gpu_ctx, len(pos))
    try:
        ids = np.arange(len(pos), dtype=np.int32)
        points.set(ids, pos=pos)
        points.set_flags(ids, bad=bad)
        zeros = np.zeros(max(N, n2), np.float32)
        table.set(0, np.zeros((N, 32), np.uint8))
        table.set_geometry(0, zeros[:N], zeros[:N], base.sigma2_1)
        cam = lambda c: dict(Rcw=c.Rcw, tcw=c.tcw, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy)
        cams = {0: cam(base.cam1)}
        for c, sc in enumerate(cands):
            table.set(c + 1, np.zeros((n2, 32), np.uint8))
            table.set_geometry(c + 1, zeros[:n2], zeros[:n2], sc.sigma2_2)
            cams[c + 1] = cam(sc.cam2)
        solvers = afv.Sim3Solver.batch(table, points, 0, [1, 2, 3], mp1, mp2, idx2, cams, False, seed=SEED, nhyp=NHYP)
        want, found_any, exhausted_any = [], False, False
        for c, s in enumerate(solvers):
            s.SetRansacParameters(0.99, MIN_INLIERS, MAX_ITS)
            while True:
                T, no_more, vb, n_in = s.iterate(5)
                want.append("%d %d %d %d %d %d %d" % (c, s.mnIterations, int(no_more), n_in, s.mnBestInliers, -1 if s.best is None else s.best,
                                                      int(T is not None)))
                if T is not None:
                    found_any = True
                    assert not vb[4] and n_in > MIN_INLIERS
                    want.append("T " + " ".join(_hx(v) for v in T.ravel()))
                    want.append("R " + " ".join(_hx(v) for v in list(s.GetEstimatedRotation().ravel()) + list(s.GetEstimatedTranslation()) +
                                                [s.GetEstimatedScale()]))
                    want.append(("i " + " ".join(str(i) for i in np.nonzero(vb)[0])).rstrip())
                if T is not None or no_more:
                    exhausted_any |= T is None
                    break
        assert found_any and exhausted_any                                             # a true candidate and a false one
        got = [l.rstrip() for l in r.stdout.splitlines()]
        assert [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in got for v in l.split()] == \
               [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in want for v in l.split()]
        assert len(got) == len(want)
    finally:
        points.close()
        table.close()

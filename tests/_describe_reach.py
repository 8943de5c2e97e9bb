"""the positions a rotated BRIEF test can land on, by an angle sweep: every pattern point rotated in 0.01 degree steps with fp32 products, one
rounding per operator, and rounded half to even - the arithmetic of k_describe (csrc/k_describe.hip) and of computeOrbDescriptor.  Shared by
tests/test_describe_reach_cpu.py (the kernel's compile-time tables against this sweep) and tests/test_gpu_describe_reach.py (the angles that
put a sample on the rim of the set)."""
import functools
import os
import re

import numpy as np

REACH = 18
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pattern():
    txt = open(os.path.join(ROOT, "anyfeature-vslam_amd", "csrc", "brief_pattern.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    p = np.array([int(v) for v in re.findall(r"-?\d+", txt)], np.int32)
    assert p.size == 1024
    return p.reshape(512, 2)


def _landings(pat, idx):
    """(ix, iy)[angle, point] for the angles idx * 0.01 degrees"""
    px, py = pat[:, 0].astype(np.float32), pat[:, 1].astype(np.float32)
    ang = (idx * np.float32(0.01)).astype(np.float32)
    t = (ang * np.float32(np.pi / 180.0)).astype(np.float32).astype(np.float64)
    c, s = np.cos(t).astype(np.float32)[:, None], np.sin(t).astype(np.float32)[:, None]
    rx = (px[None] * c).astype(np.float32) + (py[None] * -s).astype(np.float32)
    ry = (px[None] * s).astype(np.float32) + (py[None] * c).astype(np.float32)
    return np.rint(rx).astype(np.int32), np.rint(ry).astype(np.int32)


@functools.lru_cache(maxsize=None)
def sweep():
    """R[iy + 18][ix + 18], and the 64 rim angles: R less what the points below the largest radius reach is the rim; for each of its positions
    the middle of the first run of sweep angles at which a point lands there"""
    pat = pattern()
    r2 = (pat.astype(np.int64) ** 2).sum(1)
    far = r2 == r2.max()
    R = np.zeros((2 * REACH + 1, 2 * REACH + 1), bool)
    Rnear = np.zeros_like(R)
    at = {}
    for lo in range(0, 36000, 2000):
        idx = np.arange(lo, lo + 2000)
        ix, iy = _landings(pat, idx)
        assert np.abs(ix).max() <= REACH and np.abs(iy).max() <= REACH
        R[iy + REACH, ix + REACH] = True
        Rnear[iy[:, ~far] + REACH, ix[:, ~far] + REACH] = True
        for i, x, y in zip(idx.tolist(), ix[:, far][:, 0].tolist(), iy[:, far][:, 0].tolist()):
            at.setdefault((x, y), []).append(i)
    rim = R & ~Rnear
    angles = []
    for y, x in zip(*np.nonzero(rim)):
        run = at[(x - REACH, y - REACH)]
        end = next((k for k in range(1, len(run)) if run[k] != run[k - 1] + 1), len(run))
        angles.append(run[end // 2] * 0.01)
    return R, rim, sorted(angles)

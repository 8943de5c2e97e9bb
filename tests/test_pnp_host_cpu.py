"""CPU: tools/pnp_host.cpp, the scalar host program that tools/time_pnp.py times and compares the device with, answers what the
restatement tests/_pnp_ref.py answers, bit for bit, on the constructed scenes: every output array of every candidate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _pnp_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTRUCTED = S.constructed()
EXTRA = [S.build("batch_of_three", 40, 30, 8, 17, nc=3, false_rows=(1,), bad=2, unset=2, octaves=True, min_inliers=8, epsilon=0.4, nhyp=10),
         S.build("n129", 140, 129, 20, 18, octaves=True, min_inliers=10, epsilon=0.5, nhyp=6)]
SCENES = [s for s, _ in CONSTRUCTED] + EXTRA
KEYS = ("index", "count", "degenerate", "pose", "inliers", "refined", "refined_count", "refined_pose", "refined_inliers")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    so = tmp_path_factory.mktemp("pnp_host") / "pnp_host.so"
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tools", "pnp_host.cpp"),
                        "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return C.CDLL(str(so)).pnp_host


def run_host(fn, s, sigma2=None, nhyp=None, mask_words=None, stops=None):
    """tools/pnp_host.cpp on a scene -> the dict of arrays afv_frame_pnp_hypotheses answers"""
    nhyp = s.nhyp if nhyp is None else nhyp
    w = (s.N + 31) // 32 if mask_words is None else mask_words
    sigma2 = s.sigma2_host() if sigma2 is None else np.ascontiguousarray(sigma2, np.float32)
    nc, nf = s.nc, s.N
    out = dict(n=np.zeros(nc, np.int32), min_inliers=np.zeros(nc, np.int32), index=np.zeros((nc, nf), np.int32), count=np.zeros((nc, nhyp), np.int32),
               degenerate=np.zeros((nc, nhyp), np.uint8), pose=np.zeros((nc, nhyp, 12), np.float32), inliers=np.zeros((nc, nhyp, w), np.uint32),
               refined=np.zeros((nc, nhyp), np.uint8), refined_count=np.zeros((nc, nhyp), np.int32), refined_pose=np.zeros((nc, nhyp, 12), np.float32),
               refined_inliers=np.zeros((nc, nhyp, w), np.uint32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cam = np.asarray(s.cam, np.float32)
    seeds = np.asarray([s.seed + c for c in range(nc)], np.uint64)
    x, y, pos, flags, rows = (np.ascontiguousarray(a) for a in (s.x, s.y, s.store_pos, s.store_flags, s.rows))
    fn.restype = None
    fn(C.c_int(nc), C.c_int(nf), C.c_int(nhyp), C.c_int(w), None if stops is None else p(np.ascontiguousarray(stops, np.int32)), p(cam), p(seeds), C.c_int(s.min_inliers), C.c_float(s.epsilon), C.c_float(s.th2), p(x), p(y),
       p(sigma2), p(pos), p(flags), p(rows), *[p(out[k]) for k in ("n", "min_inliers") + KEYS])
    return out


@pytest.mark.parametrize("s", SCENES, ids=[s.name for s in SCENES])
def test_host_program_is_bit_equal_to_the_restatement(host_program, s):
    got = run_host(host_program, s)
    for c in range(s.nc):
        want = s.run(c)
        assert int(got["n"][c]) == want["n"] and int(got["min_inliers"][c]) == want["min_inliers"], (s.name, c)
        for k in KEYS:
            assert got[k][c].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (s.name, c, k)


def test_per_candidate_stops(host_program):
    """stops: candidate c evaluates stops[c] hypotheses; its rows up to there are those of the full run, the rest is not written"""
    s = EXTRA[0]
    full, part = run_host(host_program, s), run_host(host_program, s, stops=[4, 0, s.nhyp + 3])
    for c, stop in enumerate((4, 0, s.nhyp)):
        assert int(part["n"][c]) == int(full["n"][c]) and part["index"][c].tobytes() == full["index"][c].tobytes()
        for k in KEYS[1:]:
            assert part[k][c][:stop].tobytes() == full[k][c][:stop].tobytes(), (c, k)
            assert not part[k][c][stop:].any(), (c, k)

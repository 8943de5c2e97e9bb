"""CPU: tools/sim3opt_host.cpp, the scalar host program that tools/time_sim3opt.py times and compares the device with, answers what the
restatement tests/_sim3opt_ref.py answers, bit for bit, on every constructed scene and at the sizes around the 64 partial sums: the Sim3
doubles, the counts, the per-feature states and the trace.  The same source, built as the stand-alone program it also is with
-fsanitize=address,undefined, runs clean (no sanitizer touches code loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _sim3opt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "sim3opt_host.cpp")
INC = os.path.join(ROOT, "anyfeature-vslam_amd", "csrc")
SCENES = dict(S.every_scene())
SCENES.update({"sized_%d" % n: S.sized(n) for n in (9, 10, 11, 63, 64, 65, 128, 300)})


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    so = tmp_path_factory.mktemp("sim3opt_host") / "sim3opt_host.so"
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", INC, "-shared", "-fPIC", SRC, "-o", str(so)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(so)).sim3opt_host
    fn.restype = None
    return fn


def run_host(fn, sc):
    """tools/sim3opt_host.cpp on one scene -> (ints[9], doubles[17], state[n1])"""
    f32 = np.float32
    cam = lambda c: np.concatenate([c.Rcw, c.tcw, [c.fx, c.fy, c.cx, c.cy]]).astype(f32)
    cams = np.concatenate([cam(sc.cam1), cam(sc.cam2)])
    start = np.concatenate([sc.R12, sc.t12, [sc.s12]]).astype(f32)
    arrs = [cams, start, np.array([sc.th2], f32), np.array([int(sc.fix_scale)], np.int32), np.ascontiguousarray(sc.pos, f32),
            np.ascontiguousarray(sc.flags, np.uint8), sc.x1, sc.y1, sc.inf1, np.ascontiguousarray(sc.mp1, np.int32), sc.x2, sc.y2, sc.inf2,
            np.ascontiguousarray(sc.mp2, np.int32), np.ascontiguousarray(sc.idx2, np.int32)]
    ints, doubles, state = np.zeros(9, np.int32), np.zeros(17, np.float64), np.zeros(max(sc.n1, 1), np.uint8)
    arrs = [np.ascontiguousarray(a) for a in arrs] + [ints, doubles, state]
    fn(C.c_int(1), C.c_int(sc.n1), C.c_int(sc.n2), *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    return ints, doubles, state[:sc.n1]


def expected(r):
    ints = np.array([r.n_in, r.n_corr, r.n_bad, r.more_iterations, r.early, r.iterations[0], r.iterations[1], r.trials[0], r.trials[1]], np.int32)
    doubles = np.concatenate([r.R12, r.t12, [r.s12], r.chi2, r.lam]).astype(np.float64)
    return ints, doubles, r.state


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_program_is_bit_equal_to_the_restatement(host_program, name):
    sc = SCENES[name]
    got, want = run_host(host_program, sc), expected(sc.solve())
    assert np.array_equal(got[0], want[0]), (name, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (name, got[1], want[1])
    assert np.array_equal(got[2], want[2]), name


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "sim3opt_host"
    r = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DSIM3OPT_HOST_MAIN", "-I", INC, SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "n_in 24" in r.stdout and "early 0" in r.stdout

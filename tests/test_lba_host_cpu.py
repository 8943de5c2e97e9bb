"""CPU: tools/lba_host.cpp, the scalar host program that tools/time_lba.py times and compares the device with, answers what the
restatement tests/_lba_ref.py answers, bit for bit, on every constructed scene and on the small sized ones: the pose and point doubles,
the counts, the per-edge states and the trace.  The same source, built as the stand-alone program it also is with
-fsanitize=address,undefined, runs clean (no sanitizer touches code loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _lba_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "lba_host.cpp")
INC = os.path.join(ROOT, "anyfeature-vslam_amd", "csrc")
SCENES = dict(S.every_scene())
SCENES.update(S.small_sized())


def build_host(path):
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", INC, "-shared", "-fPIC", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(path)).lba_host
    fn.restype = None
    return fn


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("lba_host") / "lba_host.so")


def run_host(fn, sc, stop_at="scene"):
    """tools/lba_host.cpp on one scene -> (ints[8], doubles[4], kf [nf, 12], xyz [np, 3], state [ne])"""
    stop = sc.stop_at if stop_at == "scene" else stop_at
    params = np.array([sc.iterations[0], sc.iterations[1], int(sc.robust[0]), int(sc.robust[1]), int(sc.checks), -1 if stop is None else stop], np.int32)
    ints, d = np.zeros(8, np.int32), np.zeros(4, np.float64)
    kf, xyz, st = np.zeros((max(sc.nf, 1), 12)), np.zeros((max(sc.np, 1), 3)), np.zeros(max(sc.ne, 1), np.uint8)
    pad = lambda a, dt: np.ascontiguousarray(a, dt).reshape(-1) if np.size(a) else np.zeros(4, dt)
    arrs = [pad(sc.cams, np.float32), pad(sc.pos, np.float32), pad(sc.p_ok, np.uint8), pad(sc.e_pt, np.int32), pad(sc.e_kf, np.int32),
            pad(sc.obs, np.float32), params, ints, d, kf, xyz, st]
    fn(C.c_int(sc.nk), C.c_int(sc.nf), C.c_int(sc.np), C.c_int(sc.ne), *[a.ctypes.data_as(C.c_void_p) for a in arrs])
    return ints, d, kf[:sc.nf], xyz[:sc.np], st[:sc.ne]


def expected(r):
    ints = np.array(list(r.iterations) + list(r.trials) + [r.n_edges, r.n_removed_first, r.n_erase, r.stopped], np.int32)
    return ints, np.concatenate([r.chi2, r.lam]).astype(np.float64)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_program_is_bit_equal_to_the_restatement(host_program, name):
    sc = SCENES[name]
    got, r = run_host(host_program, sc), sc.solve()
    ints, doubles = expected(r)
    assert np.array_equal(got[0], ints), (name, got[0], ints)
    assert got[1].tobytes() == doubles.tobytes(), (name, got[1], doubles)
    if r.stopped == 1:           # the return at :645-647: nothing is written
        assert not got[2].any() and not got[3].any() and not got[4].any()
        return
    assert got[2].tobytes() == np.concatenate([r.R, r.t], 1).tobytes(), name
    assert got[3].tobytes() == r.xyz.tobytes(), name
    assert np.array_equal(got[4], r.state), name


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "lba_host"
    r = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DLBA_HOST_MAIN", "-I", INC, SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "n_edges 160" in r.stdout and "stopped 0" in r.stdout

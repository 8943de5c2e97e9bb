"""tools/essgraph_host.cpp for the tests: built once per session into a temporary directory, called through ctypes; and the scene file the
stand-alone program reads."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "essgraph_host.cpp")
INC = os.path.join(ROOT, "anyfeature-vslam_amd", "csrc")
MAX_L_BLOCKS, MAX_UPDATES = 131072, 2097152


def build_host(path):
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", INC, "-shared", "-fPIC", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(path))
    lib.essgraph_host.restype = None
    lib.essgraph_host_correct.restype = None
    return lib


def records(S):
    """(R [n, 3, 3], t [n, 3], s [n]) -> [n, 13] doubles: the layout of afv_sim3d"""
    n = len(S[2])
    return np.ascontiguousarray(np.concatenate([np.asarray(S[0], np.float64).reshape(n, 9), np.asarray(S[1], np.float64).reshape(n, 3),
                                                np.asarray(S[2], np.float64).reshape(n, 1)], 1))


def unrecords(a):
    a = np.asarray(a, np.float64).reshape(-1, 13)
    return a[:, :9].reshape(-1, 3, 3).copy(), a[:, 9:12].copy(), a[:, 12].copy()


class HostAnswer:
    pass


def run_host(lib, sc, max_blocks=MAX_L_BLOCKS, max_updates=MAX_UPDATES, lambda_init=1e-16):
    S, M = records(sc["S_init"]), records(sc["meas"])
    nk, ne = len(S), len(sc["v0"])
    pad = lambda a, dt: np.ascontiguousarray(a, dt).reshape(-1) if np.size(a) else np.zeros(16, dt)
    v0, v1, M = pad(sc["v0"], np.int32), pad(sc["v1"], np.int32), pad(M, np.float64)
    ints, d = np.zeros(6, np.int32), np.zeros(3, np.float64)
    So, Tiw, Swc = np.zeros((nk, 13)), np.zeros((nk, 12)), np.zeros((nk, 13))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.essgraph_host(C.c_int(nk), C.c_int(sc["fixed"]), C.c_int(ne), p(v0), p(v1), p(S), p(M), C.c_int(sc["iterations"]), C.c_double(lambda_init),
                      C.c_int(int(sc["fix_scale"])), C.c_longlong(max_blocks), C.c_longlong(max_updates), p(ints), p(d), p(So), p(Tiw), p(Swc))
    r = HostAnswer()
    r.plan = int(ints[5])
    r.iterations, r.trials, r.l_blocks, r.status, r.n_updates = (int(v) for v in ints[:5])
    r.chi2_first, r.chi2_last, r.lam = d
    r.S, r.Tiw, r.Swc = So, Tiw, Swc
    return r


def host_correct(lib, pos, flags, ids, pair, S_from, S_to):
    """the point correction of the host program over a store image: (xyz [n, 3], status [n]); pos is updated in place"""
    n = len(ids)
    ids = np.asarray(ids, np.int64)
    packed = np.ascontiguousarray(pos[ids], np.float32).reshape(-1) if n else np.zeros(3, np.float32)
    ok = np.ascontiguousarray(((flags[ids] & 1) != 0) & ((flags[ids] & 2) == 0), np.uint8) if n else np.zeros(1, np.uint8)
    pair = np.ascontiguousarray(pair, np.int32) if n else np.zeros(1, np.int32)
    xyz, st = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    A, B = np.ascontiguousarray(S_from, np.float64), np.ascontiguousarray(S_to, np.float64)
    lib.essgraph_host_correct(C.c_int(n), p(packed), p(ok), p(pair), p(A), p(B), p(xyz), p(st))
    if n:
        moved = st[:n] == 0
        pos[ids[moved]] = packed.reshape(-1, 3)[moved]
    return xyz[:n], st[:n]


def write_scene_file(path, sc, pos=None, ok=None, ref=None, lambda_init=1e-16):
    """the file the stand-alone program reads"""
    S, M = records(sc["S_init"]), records(sc["meas"])
    npts = 0 if pos is None else len(pos)
    with open(path, "wb") as f:
        f.write(np.array([len(S), sc["fixed"], len(sc["v0"]), sc["iterations"], int(sc["fix_scale"]), npts], np.int32).tobytes())
        f.write(np.float64(lambda_init).tobytes())
        f.write(S.tobytes())
        f.write(np.ascontiguousarray(sc["v0"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["v1"], np.int32).tobytes())
        f.write(M.tobytes())
        if npts:
            f.write(np.ascontiguousarray(pos, np.float32).tobytes())
            f.write(np.ascontiguousarray(ok, np.uint8).tobytes())
            f.write(np.ascontiguousarray(ref, np.int32).tobytes())

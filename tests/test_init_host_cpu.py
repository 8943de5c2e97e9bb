"""CPU: tools/initializer_host.cpp, the scalar host program that tools/time_initializer.py times and compares the device with, answers what
the restatement tests/_init_ref.py answers, bit for bit: the outputs, the trace and every per-hypothesis array."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import _init_scenes as S
from _init_check import check_against

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("init_host") / "initializer_host"
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "initializer_host.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return str(exe)


def write_scene(path, sc, calls=1):
    with open(path, "wb") as f:
        f.write(struct.pack("<4iQ5f", len(sc.x1), len(sc.x2), sc.iterations, calls, sc.seed & 0xFFFFFFFFFFFFFFFF, sc.fx, sc.fy, sc.cx, sc.cy, sc.sigma))
        for a in (sc.x1, sc.y1, sc.x2, sc.y2):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(sc.matches12, np.int32).tobytes())


def read_answer(path, afv, n1, it):
    raw = open(path, "rb").read()
    words = (n1 + 31) // 32
    out, o = {}, 0

    def take(name, dtype, shape):
        nonlocal o
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(raw, dtype, int(np.prod(shape)), o).reshape(shape).copy()
        o += n

    take("answer", np.int32, (2,)); take("R21", np.float32, (9,)); take("t21", np.float32, (3,)); take("p3d", np.float32, (n1, 3))
    take("triangulated", np.uint8, (n1,))
    out["trace"] = afv._lib.InitTrace.from_buffer_copy(raw, o)
    o += C.sizeof(afv._lib.InitTrace)
    take("score", np.float32, (2, it)); take("model", np.float32, (2, it, 9)); take("degenerate", np.uint8, (2, it))
    take("inliers", np.uint32, (2, it, words))
    assert o == len(raw)
    out["ok"], out["route"] = int(out["answer"][0]), int(out["answer"][1])
    return out


@pytest.mark.parametrize("name", ["plane", "cloud", "outliers", "low_parallax", "ambiguous", "d_ratio", "repeated", "all_repeated", "n7", "n8",
                                  "n65", "cos1", "cos51", "rh_above", "rh_below", "iter65"])
def test_host_program_is_bit_equal_to_the_restatement(afv, host_program, tmp_path, name):
    sc = S.scene(name)
    write_scene(tmp_path / "scene.bin", sc)
    r = subprocess.run([host_program, str(tmp_path / "scene.bin"), str(tmp_path / "answer.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.split()) == 3
    check_against(read_answer(tmp_path / "answer.bin", afv, len(sc.x1), sc.iterations), S.reference(name), sc, name)

"""CPU: the library exports afv_frame_pose_optimize (include/afv_hip.h, "pose optimisation"), _lib.py binds it, its records mirror the
header, NULL arguments are refused and the Python entry points exist."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    name = "afv_frame_pose_optimize"
    assert hasattr(lib, name) and name in afv._lib.SYMBOLS
    assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1]
    assert lib.afv_abi_version() == 6
    assert all(hasattr(afv.Frame, m) for m in ("PoseOptimization", "PoseOptimizationBatch"))


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    j, r = L.sized(L.PoseJob), L.sized(L.PoseResult)
    assert lib.afv_frame_pose_optimize(None, None, C.byref(j), 1, C.byref(r)) == L.EINVAL
    assert lib.afv_frame_pose_optimize(None, None, None, 1, None) == L.EINVAL
    assert lib.afv_frame_pose_optimize(None, None, C.byref(j), 0, C.byref(r)) == L.EINVAL


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    pairs = [("afv_pose_job", L.PoseJob), ("afv_pose_result", L.PoseResult)]
    names = {"lambda_": "lambda"}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for cname, st in pairs:
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, names.get(fname, fname)))
    lines += ['  printf("jobs %d\\n", AFV_POSE_MAX_JOBS);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    for cname, st in pairs:
        assert int(got[cname]) == C.sizeof(st)
        for fname, _ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)
    assert int(got["jobs"]) == L.POSE_MAX_JOBS

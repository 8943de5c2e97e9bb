"""CPU: the library exports the entry points of the new map points (include/afv_hip.h, "new map points"), _lib.py binds them, the job
record mirrors the header, and NULL arguments are refused."""
import ctypes as C
import os
import subprocess

NEW = ("afv_table_set_scale", "afv_table_triangulate")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in afv._lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1]
    assert lib.afv_abi_version() == 6
    assert all(hasattr(afv.table.DescriptorTable, m) for m in ("set_scale", "triangulate", "CreateNewMapPoints", "tri_points_jobs"))


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    one = (C.c_float * 1)()
    assert lib.afv_table_set_scale(None, 0, one, None, None, None) == L.EINVAL
    jobs = (L.TriPointsJob * 1)()
    jobs[0].struct_size = C.sizeof(L.TriPointsJob)
    ints = (C.c_int32 * 4)()
    assert lib.afv_table_triangulate(None, ints, ints, jobs, 1, ints, None, 0, None, None, None, None, None) == L.EINVAL


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    st, cname = L.TriPointsJob, "afv_tri_points_job"
    assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {',
             '  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in st._fields_:
        lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("status %d %d %d %d %d %d %d %d %d %d %d\\n", AFV_TRI_NO_MATCH, AFV_TRI_ACCEPTED, AFV_TRI_LOW_PARALLAX, AFV_TRI_W_ZERO, AFV_TRI_Z1, '
              'AFV_TRI_Z2, AFV_TRI_REPROJ1, AFV_TRI_REPROJ2, AFV_TRI_ZERO_DIST, AFV_TRI_SCALE_RATIO, AFV_TRI_NOT_FINITE);',
              '  printf("route %d %d %d\\n", AFV_TRI_ROUTE_TRIANGULATED, AFV_TRI_ROUTE_UNPROJECT_A, AFV_TRI_ROUTE_UNPROJECT_B);',
              '  printf("pairs %d\\n", AFV_TRI_MAX_PAIRS);', '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(st)
    for fname, _ in st._fields_:
        assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, fname
    assert got["status"].split() == [str(v) for v in range(len(L.TRI_STATUS))]
    assert got["route"].split() == [str(v) for v in range(len(L.TRI_ROUTE))]
    assert int(got["pairs"]) == L.TRI_MAX_PAIRS and int(got["abi"]) == 6


def test_status_names_agree_with_the_restatement(afv):
    import _tri_ref as R
    assert tuple(afv._lib.TRI_STATUS) == tuple(R.STATUS_NAMES)
    assert (R.TRIANGULATED, R.UNPROJECT_A, R.UNPROJECT_B) == (0, 1, 2)

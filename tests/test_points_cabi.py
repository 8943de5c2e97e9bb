"""CPU: the library exports the resident map-point entry points (include/afv_hip.h, "resident map points"), _lib.py binds them, their
records mirror the header, and NULL arguments are refused."""
import ctypes as C
import os
import subprocess

NEW = ("afv_points_create", "afv_points_destroy", "afv_points_set", "afv_points_set_flags", "afv_points_set_descriptors",
       "afv_points_set_descriptors_from_table", "afv_points_get", "afv_frame_set_pose", "afv_frame_search_points", "afv_frame_fuse_points",
       "afv_frame_project_points")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in afv._lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1]
    assert lib.afv_abi_version() == 6
    assert hasattr(afv, "MapPoints") and all(hasattr(afv.Frame, m) for m in (
        "set_pose", "isInFrustum", "SearchLocalPoints", "SearchByProjectionLast", "SearchByProjectionReloc", "FusePoints", "project_points"))


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    h = C.c_void_p()
    assert lib.afv_points_create(None, 16, 32, 0, C.byref(h)) == L.EINVAL
    lib.afv_points_destroy(None)
    assert lib.afv_points_set(None, None, 0, None, None, None, None, None, None, None) == L.EINVAL
    assert lib.afv_points_set_flags(None, None, 0, None, None) == L.EINVAL
    assert lib.afv_points_set_descriptors(None, None, 0, None) == L.EINVAL
    assert lib.afv_points_set_descriptors_from_table(None, None, 0, None, None, None) == L.EINVAL
    assert lib.afv_points_get(None, None, 0, None, None, None, None, None, None, None, None, None) == L.EINVAL
    assert lib.afv_frame_set_pose(None, None, None, None, 1.0, 1.0, 0.0, 0.0, 0.0) == L.EINVAL
    s = L.sized(L.PointSearch)
    assert lib.afv_frame_search_points(None, C.byref(s), None, None, None, None) == L.EINVAL
    assert lib.afv_frame_fuse_points(None, C.byref(s), 1, None, None) == L.EINVAL
    assert lib.afv_frame_project_points(None, C.byref(s), None) == L.EINVAL


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    pairs = [("afv_point_search", L.PointSearch), ("afv_point_projection", L.PointProjection)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for cname, st in pairs:
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("flavours %d %d %d %d\\n", AFV_PT_FRUSTUM, AFV_PT_LASTFRAME, AFV_PT_RELOC, AFV_PT_FUSE);',
              '  printf("cap %d\\n", AFV_POINTS_MAX_CAPACITY);', '  return 0;', '}']
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
    assert got["flavours"].split() == [str(v) for v in (L.PT_FRUSTUM, L.PT_LASTFRAME, L.PT_RELOC, L.PT_FUSE)]
    assert int(got["cap"]) == L.POINTS_MAX_CAPACITY

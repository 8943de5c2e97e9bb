"""CPU: the library exports the entry points of "fusing map points into keyframes of the table" (include/afv_hip.h), _lib.py binds them, the
record sizes and caps are the header's, the wrappers exist, every refusal that needs no table answers AFV_EINVAL with the outputs untouched
(the refusals that need a table and a store are in tests/test_gpu_kffuse.py), and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = (("afv_table_set_camera", 2), ("afv_table_set_pose", 10), ("afv_table_set_map_points", 3), ("afv_table_get_map_points", 3),
       ("afv_table_fuse_points", 8))


def test_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name, nargs in NEW:
        assert hasattr(lib, name) and name in afv._lib.SYMBOLS
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == nargs
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    for m in ("set_camera", "set_pose", "set_map_points", "get_map_points", "FusePoints", "FusePointsSim3", "SearchInNeighborsFuse", "SearchAndFuse",
              "decompose_scw"):
        assert hasattr(afv.table.DescriptorTable, m), m


def test_records_and_caps_match_the_header(afv, tmp_path):
    L = afv._lib
    pairs = [("afv_table_camera", L.TableCamera), ("afv_table_fuse_pose", L.TableFusePose), ("afv_table_fuse_job", L.TableFuseJob)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {',
             '  printf("caps %d %d %d\\n", AFV_KFFUSE_MAX_TARGETS, AFV_KFFUSE_MAX_QUERIES, AFV_ABI_VERSION);']
    for cname, st in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert out[0].split() == ["caps", str(L.KFFUSE_MAX_TARGETS), str(L.KFFUSE_MAX_QUERIES), "6"] == ["caps", "64", "1048576", "6"]
    got = dict(l.split() for l in out[1:])
    for cname, st in pairs:
        assert int(got[cname]) == C.sizeof(st), (cname, got[cname], C.sizeof(st))
        for fname, _ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)
    assert [C.sizeof(st) for _, st in pairs] == [36, 60, 48]
    for st in (L.TableCamera, L.TableFuseJob):
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    assert L.KFFUSE_STATUS == {"invalid": 0, "in_keyframe": 1, "not_in_view": 2, "no_feature": 3, "free": 4, "occupant_bad": 5, "replace": 6}


def test_refusals_without_a_table_leave_the_outputs_untouched(afv):
    L = afv._lib
    lib = L.load()
    cam = L.sized(L.TableCamera)
    assert lib.afv_table_set_camera(None, C.byref(cam)) == L.EINVAL
    f3 = np.zeros(9, np.float32)
    assert lib.afv_table_set_pose(None, 0, L.ptr(f3), L.ptr(f3), L.ptr(f3), 1.0, 1.0, 0.0, 0.0, 0.0) == L.EINVAL
    ids = np.zeros(4, np.int32)
    assert lib.afv_table_set_map_points(None, 0, L.ptr(ids)) == L.EINVAL
    assert lib.afv_table_get_map_points(None, 0, L.ptr(ids)) == L.EINVAL and np.all(ids == 0)
    jobs = (L.TableFuseJob * 1)()
    jobs[0].struct_size = C.sizeof(L.TableFuseJob)
    best, occ = np.full(4, 77, np.int32), np.full(4, 77, np.int32)
    st, nf = np.full(4, 0xA5, np.uint8), np.full(1, 77, np.int32)
    for nt in (1, 0, -1, 65):
        assert lib.afv_table_fuse_points(None, None, jobs, nt, L.ptr(best), L.ptr(occ), L.ptr(st), L.ptr(nf)) == L.EINVAL
    assert np.all(best == 77) and np.all(occ == 77) and np.all(st == 0xA5) and np.all(nf == 77)


def test_decompose_scw_is_the_restatement(afv):
    import _kffuse_ref as K
    import _points_scenes as S
    for k in range(5):
        rs = np.random.RandomState(k)
        Scw = np.eye(4, dtype=np.float32)
        Scw[:3, :3] = S.rotation(*rs.uniform(-0.5, 0.5, 3)) * np.float32(rs.uniform(0.5, 2.5))
        Scw[:3, 3] = rs.uniform(-2, 2, 3)
        got, want = afv.table.DescriptorTable.decompose_scw(Scw), K.decompose_scw(Scw)
        for a, b in zip(got, want):
            assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
        assert np.array_equal(got[1], Scw[:3, 3])   # the kept quirk: tcw is not divided by scw

"""CPU: the library exports afv_table_refresh_points (include/afv_hip.h, "Refresh of resident map points"), _lib.py binds it, the records
mirror the header, the package exports RefreshMapPoints / UpdateNormalAndDepth / ComputeDistinctiveDescriptors, every refusal that needs
no table answers AFV_EINVAL with the poisoned outputs untouched (the refusals that need a table and a store are in
tests/test_gpu_refresh.py), and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    name = "afv_table_refresh_points"
    assert hasattr(lib, name) and name in afv._lib.SYMBOLS
    assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == 16
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.RefreshMapPoints is afv.refresh.RefreshMapPoints and afv.UpdateNormalAndDepth is afv.refresh.UpdateNormalAndDepth
    assert afv.ComputeDistinctiveDescriptors is afv.refresh.ComputeDistinctiveDescriptors
    assert afv.RefreshAfterBundleAdjustment is afv.refresh.RefreshAfterBundleAdjustment and afv.refresh.edge_arrays is afv.lba.edge_arrays


def test_camera_centre_is_the_float_expression_of_set_pose(afv):
    import _points_ref as P
    rng = np.random.RandomState(2)
    for _ in range(10):
        R, t = np.linalg.qr(rng.randn(3, 3))[0], rng.randn(3) * 3
        assert afv.refresh.camera_centre(R, t).tobytes() == P.twc(R, t).tobytes()


def test_refusals_without_a_table_leave_the_outputs_untouched(afv):
    L = afv._lib
    lib = L.load()
    prm = L.sized(L.RefreshParams)
    prm.descriptors, prm.normals = 1, 1
    ints, floats = np.zeros(8, np.int32), np.zeros(8, np.float32)
    status, best, med = (np.full(4, 0x5A5A5A5A, np.int32) for _ in range(3))
    out = L.sized(L.RefreshOut)
    out.status, out.best_obs, out.best_median = status.ctypes.data, best.ctypes.data, med.ctypes.data
    p = L.ptr

    def call(t=None, pts=None, slots=ints, nk=2, cen=floats, mx=floats, bad=None, ids=ints, npts=2, ref=ints, op=ints, ok=ints, oi=ints, ne=2, prm=prm,
             out=out):
        a = lambda v: p(v) if isinstance(v, np.ndarray) else v
        return lib.afv_table_refresh_points(t, pts, a(slots), nk, a(cen), a(mx), a(bad), a(ids), npts, a(ref), a(op), a(ok), a(oi), ne,
                                            None if prm is None else C.byref(prm), None if out is None else C.byref(out))

    # no table, no store, whatever else is right or wrong: refused before anything is read
    assert call() == L.EINVAL
    for bad in (dict(slots=None), dict(cen=None), dict(mx=None), dict(ids=None), dict(ref=None), dict(op=None), dict(ok=None), dict(oi=None),
                dict(prm=None), dict(out=None), dict(nk=L.LBA_MAX_KF + 1), dict(nk=-1), dict(npts=L.LBA_MAX_POINTS + 1), dict(npts=-1),
                dict(ne=L.LBA_MAX_EDGES + 1), dict(ne=-1)):
        assert call(**bad) == L.EINVAL, bad
    assert all(np.all(a == 0x5A5A5A5A) for a in (status, best, med))


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    records = ((L.RefreshParams, "afv_refresh_params", 12), (L.RefreshOut, "afv_refresh_out", 32))
    for st, _, _ in records:
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for st, cname, _ in records:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("states %d %d %d %d %d\\n", AFV_REFRESH_DONE, AFV_REFRESH_SKIPPED, AFV_REFRESH_NO_OBSERVATIONS, AFV_REFRESH_NO_REF, '
              'AFV_REFRESH_BAD_DISTANCE);', '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    for st, cname, size in records:
        assert int(got[cname]) == C.sizeof(st) == size, cname
        for fname, _ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)
    assert [int(v) for v in got["states"].split()] == [L.REFRESH_DONE, L.REFRESH_SKIPPED, L.REFRESH_NO_OBSERVATIONS, L.REFRESH_NO_REF,
                                                       L.REFRESH_BAD_DISTANCE] == [0, 1, 2, 3, 4]
    import _refresh_ref as R
    assert (R.DONE, R.SKIPPED, R.NO_OBSERVATIONS, R.NO_REF, R.BAD_DISTANCE) == (0, 1, 2, 3, 4)
    assert int(got["abi"]) == 6

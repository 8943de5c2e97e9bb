"""CPU: the library exports afv_table_bundle_adjust (include/afv_hip.h, "Bundle adjustment"), _lib.py binds it, the records mirror the
header, the package exports LocalBundleAdjustment / BundleAdjustment, every refusal that needs no table answers AFV_EINVAL with the
poisoned outputs untouched (the refusals that need a table and a store are in tests/test_gpu_lba.py), and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    name = "afv_table_bundle_adjust"
    assert hasattr(lib, name) and name in afv._lib.SYMBOLS
    assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == 18
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.LocalBundleAdjustment is afv.lba.LocalBundleAdjustment and afv.BundleAdjustment is afv.lba.BundleAdjustment


def test_refusals_without_a_table_leave_the_outputs_untouched(afv):
    L = afv._lib
    lib = L.load()
    cams = (L.LbaCam * 2)()
    for c in cams:
        c.struct_size = C.sizeof(L.LbaCam)
    prm = L.sized(L.LbaParams)
    prm.iterations[0], prm.iterations[1], prm.robust[0], prm.checks, prm.write_points = 5, 10, 1, 1, 1
    ints = np.zeros(8, np.int32)
    res = L.LbaResult()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    kf, xyz, state = np.full(24, 7.5), np.full(24, 7.5), np.full(8, 0xA5, np.uint8)
    p = L.ptr

    def call(t=None, pts=None, slots=ints, nk=2, nf=1, cams=cams, ids=ints, npts=2, op=ints, ok=ints, oi=ints, ne=2, prm=prm, res=res, kf=kf, xyz=xyz,
             state=state):
        a = lambda v: p(v) if isinstance(v, np.ndarray) else v
        return lib.afv_table_bundle_adjust(t, pts, a(slots), nk, nf, cams, a(ids), npts, a(op), a(ok), a(oi), ne, None if prm is None else C.byref(prm),
                                           None, None if res is None else C.byref(res), a(kf), a(xyz), a(state))

    # no table, no store, whatever else is right or wrong: refused before anything is read
    assert call() == L.EINVAL
    for bad in (dict(slots=None), dict(cams=None), dict(ids=None), dict(op=None), dict(ok=None), dict(oi=None), dict(prm=None), dict(res=None),
                dict(kf=None), dict(xyz=None), dict(state=None), dict(nk=L.LBA_MAX_KF + 1), dict(nf=L.LBA_MAX_FREE + 1), dict(nf=3), dict(nk=-1),
                dict(npts=L.LBA_MAX_POINTS + 1), dict(ne=L.LBA_MAX_EDGES + 1), dict(ne=-1)):
        assert call(**bad) == L.EINVAL, bad
    assert bytes(res) == b"\xa5" * C.sizeof(res) and np.all(kf == 7.5) and np.all(xyz == 7.5) and np.all(state == 0xA5)


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    records = ((L.LbaCam, "afv_lba_cam", 72), (L.LbaParams, "afv_lba_params", 32), (L.LbaResult, "afv_lba_result", 64))
    rename = {"lam": "lambda"}
    for st in (L.LbaCam, L.LbaParams):
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for st, cname, _ in records:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, rename.get(fname, fname)))
    lines += ['  printf("states %d %d %d %d\\n", AFV_LBA_EDGE_DROPPED, AFV_LBA_EDGE_KEPT, AFV_LBA_EDGE_REMOVED_KEPT, AFV_LBA_EDGE_ERASE);',
              '  printf("caps %d %d %d %d\\n", AFV_LBA_MAX_FREE, AFV_LBA_MAX_KF, AFV_LBA_MAX_POINTS, AFV_LBA_MAX_EDGES);',
              '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
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
    assert [int(v) for v in got["states"].split()] == [L.LBA_EDGE_DROPPED, L.LBA_EDGE_KEPT, L.LBA_EDGE_REMOVED_KEPT, L.LBA_EDGE_ERASE] == [0, 1, 2, 3]
    assert [int(v) for v in got["caps"].split()] == [L.LBA_MAX_FREE, L.LBA_MAX_KF, L.LBA_MAX_POINTS, L.LBA_MAX_EDGES] == [64, 256, 32768, 262144]
    assert int(got["abi"]) == 6

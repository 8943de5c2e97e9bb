"""CPU: the library exports afv_essential_graph and afv_points_correct_sim3 (include/afv_hip.h, "Essential graph"), _lib.py binds them, the
records mirror the header, the package exports OptimizeEssentialGraph, essential_graph_edges and MapPoints.correct_sim3, a call
without a context answers AFV_EINVAL with the poisoned outputs untouched (that is the only refusal a machine without a device can reach:
all others are in tests/test_gpu_essgraph.py), and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name, nargs in (("afv_essential_graph", 18), ("afv_points_correct_sim3", 8)):
        assert hasattr(lib, name) and name in afv._lib.SYMBOLS
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == nargs
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.OptimizeEssentialGraph is afv.essgraph.OptimizeEssentialGraph and afv.essential_graph_edges is afv.essgraph.essential_graph_edges
    assert callable(afv.MapPoints.correct_sim3)


def test_refusals_without_a_context_leave_the_outputs_untouched(afv):
    L = afv._lib
    lib = L.load()
    prm = L.sized(L.EssParams)
    prm.iterations, prm.lambda_init, prm.fix_scale, prm.write_points = 20, 1e-16, 0, 1
    ints = np.zeros(8, np.int32)
    S = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64), (4, 1))
    res = L.EssResult()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    S_out, Tiw, xyz, st = np.full((4, 13), 7.5), np.full((4, 12), 7.5), np.full((4, 3), 7.5), np.full(4, 0xA5, np.uint8)
    p = L.ptr

    def call(ctx=None, pts=None, S=S, nk=4, fixed=0, v0=ints, v1=ints, M=S, ne=2, prm=prm, ids=ints, ref=ints, npts=2, res=res, S_out=S_out, Tiw=Tiw,
             xyz=xyz, st=st):
        a = lambda v: p(v) if isinstance(v, np.ndarray) else v
        return lib.afv_essential_graph(ctx, pts, a(S), nk, fixed, a(v0), a(v1), a(M), ne, None if prm is None else C.byref(prm), a(ids), a(ref), npts,
                                       None if res is None else C.byref(res), a(S_out), a(Tiw), a(xyz), a(st))

    # no context: refused at the first test, before anything is read.  Nothing else of the argument check can be reached without a context,
    # which needs a device: every other refusal (counts, NULL arguments, ranges) is in tests/test_gpu_essgraph.py
    assert call() == L.EINVAL
    assert call(S=None, prm=None, res=None) == L.EINVAL
    assert bytes(res) == b"\xa5" * C.sizeof(res) and np.all(S_out == 7.5) and np.all(Tiw == 7.5) and np.all(xyz == 7.5) and np.all(st == 0xA5)
    assert lib.afv_points_correct_sim3(None, p(ints), 2, p(ints), p(S), p(S), 4, p(st)) == L.EINVAL and np.all(st == 0xA5)


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    records = ((L.Sim3d, "afv_sim3d", 104), (L.EssParams, "afv_ess_params", 24), (L.EssResult, "afv_ess_result", 40))
    rename = {"lam": "lambda"}
    assert L.EssParams._fields_[0][0] == "struct_size" and L.sized(L.EssParams).struct_size == C.sizeof(L.EssParams)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for st, cname, _ in records:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, rename.get(fname, fname)))
    lines += ['  printf("status %d %d %d\\n", AFV_ESS_OK, AFV_ESS_NOT_FINITE, AFV_ESS_EMPTY);',
              '  printf("points %d %d %d\\n", AFV_POINT_MOVED, AFV_POINT_BAD_OR_UNSET, AFV_POINT_NO_PAIR);',
              '  printf("caps %d %d %d %d\\n", AFV_ESS_MAX_KF, AFV_ESS_MAX_EDGES, AFV_ESS_MAX_L_BLOCKS, AFV_ESS_MAX_UPDATES);',
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
    assert [int(v) for v in got["status"].split()] == [L.ESS_OK, L.ESS_NOT_FINITE, L.ESS_EMPTY] == [0, 1, 2]
    assert [int(v) for v in got["points"].split()] == [L.POINT_MOVED, L.POINT_BAD_OR_UNSET, L.POINT_NO_PAIR] == [0, 1, 2]
    assert [int(v) for v in got["caps"].split()] == [L.ESS_MAX_KF, L.ESS_MAX_EDGES, L.ESS_MAX_L_BLOCKS, L.ESS_MAX_UPDATES] == [4096, 65536, 131072, 2097152]
    assert int(got["abi"]) == 6

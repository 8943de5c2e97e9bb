"""CPU: the library exports afv_table_optimize_sim3 and afv_table_set_inf (include/afv_hip.h, "OptimizeSim3"), _lib.py binds them, the
job and result records mirror the header, NULL arguments are refused and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"afv_table_optimize_sim3": 11, "afv_table_set_inf": 3}


def test_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name, nargs in NAMES.items():
        assert hasattr(lib, name) and name in afv._lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == nargs, name
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.OptimizeSim3 is afv.sim3.OptimizeSim3 and afv.OptimizeSim3Batch is afv.sim3.OptimizeSim3Batch
    assert hasattr(afv.table.DescriptorTable, "set_inf")


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    jobs = (L.Sim3OptJob * 1)()
    jobs[0].struct_size = C.sizeof(L.Sim3OptJob)
    res = (L.Sim3OptResult * 1)()
    ints = (C.c_int32 * 8)()
    state = (C.c_uint8 * 8)()
    # no table, no store: refused before anything is read
    assert lib.afv_table_optimize_sim3(None, None, ints, ints, jobs, 1, ints, ints, ints, res, state) == L.EINVAL
    assert lib.afv_table_optimize_sim3(None, None, None, None, None, 0, None, None, None, None, None) == L.EINVAL
    assert lib.afv_table_set_inf(None, 0, ints) == L.EINVAL


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    records = ((L.Sim3OptJob, "afv_sim3opt_job", 192), (L.Sim3OptResult, "afv_sim3opt_result", 176))
    rename = {"lam": "lambda"}
    assert L.Sim3OptJob._fields_[0][0] == "struct_size" and L.sized(L.Sim3OptJob).struct_size == C.sizeof(L.Sim3OptJob)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for st, cname, _ in records:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, rename.get(fname, fname)))
    lines += ['  printf("states %d %d %d %d %d\\n", AFV_SIM3OPT_NO_MATCH, AFV_SIM3OPT_NOT_EDGE, AFV_SIM3OPT_KEPT, AFV_SIM3OPT_REMOVED_FIRST, '
              'AFV_SIM3OPT_REMOVED_SECOND);', '  printf("limit %d\\n", AFV_SIM3_MAX_CANDIDATES);', '  printf("abi %d\\n", AFV_ABI_VERSION);',
              '  return 0;', '}']
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
    assert [int(v) for v in got["states"].split()] == [L.SIM3OPT_NO_MATCH, L.SIM3OPT_NOT_EDGE, L.SIM3OPT_KEPT, L.SIM3OPT_REMOVED_FIRST,
                                                       L.SIM3OPT_REMOVED_SECOND] == [0, 1, 2, 3, 4]
    assert int(got["limit"]) == L.SIM3_MAX_CANDIDATES == 64
    assert int(got["abi"]) == 6

"""CPU: the library exports afv_table_sim3_hypotheses (include/afv_hip.h, "Sim3Solver"), _lib.py binds it, the job record mirrors the
header, NULL arguments are refused and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "afv_table_sim3_hypotheses"


def test_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    assert hasattr(lib, NAME) and NAME in afv._lib.SYMBOLS
    assert getattr(lib, NAME).argtypes == afv._lib.SYMBOLS[NAME][1] and len(afv._lib.SYMBOLS[NAME][1]) == 21
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.Sim3Solver is afv.sim3.Sim3Solver
    assert all(hasattr(afv.Sim3Solver, m) for m in ("batch", "SetRansacParameters", "iterate", "find", "GetEstimatedRotation",
                                                    "GetEstimatedTranslation", "GetEstimatedScale"))


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    jobs = (L.Sim3Job * 1)()
    jobs[0].struct_size = C.sizeof(L.Sim3Job)
    ints = (C.c_int32 * 8)()
    out = (C.c_float * 64)()
    # no table, no store: refused before anything is read
    assert lib.afv_table_sim3_hypotheses(None, None, ints, ints, jobs, 1, ints, ints, None, ints, 1, 1, ints, ints, ints, out, out, out, None, None,
                                         None) == L.EINVAL
    assert lib.afv_table_sim3_hypotheses(None, None, None, None, None, 0, None, None, None, None, 0, 0, None, None, None, None, None, None, None,
                                         None, None) == L.EINVAL


def test_record_mirror_matches_the_header(afv, tmp_path):
    L = afv._lib
    st, cname = L.Sim3Job, "afv_sim3_job"
    assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {',
             '  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in st._fields_:
        lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("limits %d %d %d\\n", AFV_SIM3_MAX_CANDIDATES, AFV_SIM3_MAX_HYPOTHESES, AFV_SIM3_MAX_MASK_WORDS);',
              '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(st) == 144
    for fname, _ in st._fields_:
        assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, fname
    assert [int(v) for v in got["limits"].split()] == [L.SIM3_MAX_CANDIDATES, L.SIM3_MAX_HYPOTHESES, L.SIM3_MAX_MASK_WORDS] == [64, 1024, 256]
    assert int(got["abi"]) == 6

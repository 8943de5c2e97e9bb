"""CPU: the library exports afv_frame_initializer (include/afv_hip.h, "Initializer"), _lib.py binds it, the record mirrors match the
header, the limits are right, NULL and out-of-range arguments are refused and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "afv_frame_initializer"


def test_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    assert hasattr(lib, NAME) and NAME in afv._lib.SYMBOLS
    assert getattr(lib, NAME).argtypes == afv._lib.SYMBOLS[NAME][1] and len(afv._lib.SYMBOLS[NAME][1]) == 16
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.Initializer is afv.initializer.Initializer
    assert all(hasattr(afv.Initializer, m) for m in ("Initialize", "hypotheses", "parallax_degrees"))
    assert callable(afv.initializer.initialize)


def test_null_and_out_of_range_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    job = L.sized(L.InitJob)
    job.iterations, job.fx, job.fy, job.cx, job.cy, job.sigma = 8, 500.0, 500.0, 320.0, 240.0, 1.0
    ints = (C.c_int32 * 8)()
    out = (C.c_float * 64)()
    ok, route = C.c_int32(77), C.c_int32(77)
    # no frames: refused before anything is read or written
    assert lib.afv_frame_initializer(None, None, C.byref(job), ints, C.byref(ok), C.byref(route), out, out, out, out, None, None, None, None,
                                     None, 0) == L.EINVAL
    assert lib.afv_frame_initializer(None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0) == L.EINVAL
    job.iterations = L.INIT_MAX_ITERATIONS + 1
    assert lib.afv_frame_initializer(None, None, C.byref(job), ints, C.byref(ok), C.byref(route), out, out, out, out, None, None, None, None,
                                     None, -1) == L.EINVAL
    assert (ok.value, route.value) == (77, 77) and not any(out)


def test_record_mirrors_match_the_header(afv, tmp_path):
    L = afv._lib
    records = ((L.InitJob, "afv_init_job", 36), (L.InitTrace, "afv_init_trace", 640))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {']
    for st, cname, _ in records:
        assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("limits %d %d %d\\n", AFV_INIT_MAX_ITERATIONS, AFV_INIT_MAX_MOTIONS, AFV_INIT_MAX_MASK_WORDS);',
              '  printf("routes %d %d\\n", AFV_INIT_ROUTE_H, AFV_INIT_ROUTE_F);',
              '  printf("reasons %d %d %d %d %d %d %d\\n", AFV_INIT_OK, AFV_INIT_TOO_FEW_MATCHES, AFV_INIT_D_RATIO, AFV_INIT_AMBIGUOUS, '
              'AFV_INIT_PARALLAX, AFV_INIT_MIN_TRIANGULATED, AFV_INIT_MIN_GOOD);',
              '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    for st, cname, size in records:
        assert int(got[cname]) == C.sizeof(st) == size
        for fname, _ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, fname
    assert [int(v) for v in got["limits"].split()] == [L.INIT_MAX_ITERATIONS, L.INIT_MAX_MOTIONS, L.INIT_MAX_MASK_WORDS] == [1024, 8, 256]
    assert [int(v) for v in got["routes"].split()] == [L.INIT_ROUTE_H, L.INIT_ROUTE_F] == [0, 1]
    assert [int(v) for v in got["reasons"].split()] == list(range(len(L.INIT_REASON))) == list(range(7))
    assert int(got["abi"]) == 6


def test_reason_names_are_the_restatement_s(afv):
    import _init_ref as R
    assert tuple(afv._lib.INIT_REASON) == tuple(R.REASONS)
    assert (afv._lib.INIT_ROUTE_H, afv._lib.INIT_ROUTE_F) == (R.ROUTE_H, R.ROUTE_F)

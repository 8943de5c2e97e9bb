"""CPU: the library exports afv_frame_pnp_hypotheses (include/afv_hip.h, "PnPsolver"), _lib.py binds it, the job record mirrors the
header, NULL arguments are refused, the Python class refuses what it must refuse without a device and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "afv_frame_pnp_hypotheses"


def test_symbol_is_exported_and_bound(afv):
    lib = afv._lib.load()
    assert hasattr(lib, NAME) and NAME in afv._lib.SYMBOLS
    assert getattr(lib, NAME).argtypes == afv._lib.SYMBOLS[NAME][1] and len(afv._lib.SYMBOLS[NAME][1]) == 20
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.PnPsolver is afv.pnp.PnPsolver
    assert all(hasattr(afv.PnPsolver, m) for m in ("batch", "SetRansacParameters", "iterate", "find"))
    assert hasattr(afv.Frame, "PnPsolverBatch")


def test_null_arguments_are_refused(afv):
    L = afv._lib
    lib = L.load()
    jobs = afv.pnp.pnp_jobs([1], 10, 0.5, 5.991)
    ints = (C.c_int32 * 64)()
    out = (C.c_float * 64)()
    # no frame, no store: refused before anything is read
    assert lib.afv_frame_pnp_hypotheses(None, None, jobs, 1, ints, 1, 1, ints, ints, ints, ints, out, out, out, out, ints, out, out, None, None) == L.EINVAL
    assert lib.afv_frame_pnp_hypotheses(*([None] * 3 + [0, None, 0, 0] + [None] * 13)) == L.EINVAL


def test_record_mirror_matches_the_header(afv, tmp_path):
    L = afv._lib
    st, cname = L.PnpJob, "afv_pnp_job"
    assert st._fields_[0][0] == "struct_size" and L.sized(st).struct_size == C.sizeof(st)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {',
             '  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in st._fields_:
        lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  printf("limits %d %d %d\\n", AFV_PNP_MAX_CANDIDATES, AFV_PNP_MAX_HYPOTHESES, AFV_PNP_MAX_MASK_WORDS);',
              '  printf("abi %d\\n", AFV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(st) == 24
    for fname, _ in st._fields_:
        assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, fname
    assert [int(v) for v in got["limits"].split()] == [L.PNP_MAX_CANDIDATES, L.PNP_MAX_HYPOTHESES, L.PNP_MAX_MASK_WORDS] == [64, 1024, 256]
    assert int(got["abi"]) == 6


def solver(afv, nhyp=8, n=20, counts=None, given=(10, 0.5, 5.991)):
    z = lambda *shape, dtype=np.int32: np.zeros(shape, dtype)
    count = z(nhyp) if counts is None else np.asarray(counts, np.int32)
    return afv.PnPsolver(n, 10, np.arange(n, dtype=np.int32), count, z(nhyp, dtype=np.uint8), z(nhyp, 12, dtype=np.float32),
                         z(nhyp, 1, dtype=np.uint32), z(nhyp, dtype=np.uint8), z(nhyp), z(nhyp, 12, dtype=np.float32), z(nhyp, 1, dtype=np.uint32),
                         n, given)


def test_the_class_refuses_without_a_device(afv):
    s = solver(afv)
    assert s.mRansacMinInliers == 10 and s.mRansacMaxIts == 8   # epsilon 0.5 at N = 20: 35 iterations wanted, 8 evaluated
    for kw in (dict(minInliers=9), dict(epsilon=0.4), dict(th2=6.0), dict(minSet=5), dict(maxIterations=9)):
        args = dict(probability=0.99, minInliers=10, maxIterations=8, minSet=4, epsilon=0.5, th2=5.991)
        args.update(kw)
        with pytest.raises(ValueError):
            s.SetRansacParameters(**args)
    s.SetRansacParameters(0.99, 10, 5, 4, 0.5, 5.991)
    assert s.mRansacMaxIts == 5
    T, no_more, vb, n = s.iterate(5)
    assert T is None and no_more and n == 0 and not vb.any() and s.mnIterations == 5
    with pytest.raises(IndexError):   # Q1: every later call still runs its own five hypotheses
        s.iterate(5)
    with pytest.raises(ValueError):   # the device's mRansacMinInliers must be the host's
        afv.PnPsolver(40, 10, *[np.zeros(1, np.int32)] * 9, 40, (10, 0.5, 5.991))
    few = solver(afv, n=6)
    assert few.iterate(5)[:2] == (None, True) and few.mnIterations == 0


def test_ransac_parameters_of_the_class_at_the_references_constants(afv):
    """include/Tracking.h:323-328 (0.99, 10, 300, 4, 0.5, 5.991): mRansacMaxIts = 35 at N = 100 and 14 at N = 15, computed by the package's
    own host mathematics (tests/test_pnp_ref_cpu.py asserts the same of the restatement's)"""
    for n, n_min, want in ((100, 50, 35), (15, 10, 14)):
        z = lambda *shape, dtype=np.int32: np.zeros(shape, dtype)
        s = afv.PnPsolver(n, n_min, np.arange(n, dtype=np.int32), z(300), z(300, dtype=np.uint8), z(300, 12, dtype=np.float32),
                          z(300, 4, dtype=np.uint32), z(300, dtype=np.uint8), z(300), z(300, 12, dtype=np.float32), z(300, 4, dtype=np.uint32), n,
                          (10, 0.5, 5.991))
        s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
        assert (s.mRansacMinInliers, s.mRansacMaxIts) == (n_min, want)

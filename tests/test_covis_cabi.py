"""CPU: the C-ABI of include/afv_covis.h - the symbols are exported and bound by covisibility.py's own table (not by _lib.SYMBOLS, whose set is
pinned to afv_hip.h and afv_akaze.h by tests/test_cabi.py), the header compiles as C11, the ctypes record matches it, the caps match, the ABI
revision is unchanged, and the refusals that need no table answer AFV_EINVAL with the outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "afv_covis.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(afv_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_exported_and_bound_by_the_modules_own_table(afv):
    cv = afv.covisibility
    declared = _declared()
    assert declared == ["afv_table_covis_votes", "afv_table_local_points"]
    assert sorted(cv.SYMBOLS) == declared
    lib = cv.bind()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == cv.SYMBOLS[name][1] and fn.restype is cv.SYMBOLS[name][0]
        assert name not in afv._lib.SYMBOLS
    assert lib.afv_abi_version() == 6 == afv._lib.ABI_VERSION
    assert afv.CovisibilityGraph is cv.CovisibilityGraph and afv.covisibility_votes is cv.covisibility_votes and afv.local_points is cv.local_points


def test_header_compiles_as_c11_and_the_record_matches(afv, tmp_path):
    cv = afv.covisibility
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_covis.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(afv_covis_query));']
    for fname, _ in cv.CovisQuery._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(afv_covis_query, %s));' % (fname, fname))
    for cap in ("AFV_COVIS_MAX_IDS", "AFV_COVIS_MAX_QUERIES", "AFV_COVIS_MAX_LOCAL", "AFV_COVIS_MAX_KF", "AFV_COVIS_MAX_CAP", "AFV_COVIS_QUERY_SLOT",
                "AFV_COVIS_QUERY_IDS", "AFV_ABI_VERSION"):
        lines.append('  printf("%s %%d\\n", (int)%s);' % (cap, cap))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cv.CovisQuery)
    for fname, _ in cv.CovisQuery._fields_:
        assert int(got[fname]) == getattr(cv.CovisQuery, fname).offset, fname
    assert cv.CovisQuery._fields_[0][0] == "struct_size"
    assert (int(got["AFV_COVIS_MAX_IDS"]), int(got["AFV_COVIS_MAX_QUERIES"]), int(got["AFV_COVIS_MAX_LOCAL"]), int(got["AFV_COVIS_MAX_KF"]),
            int(got["AFV_COVIS_MAX_CAP"])) == (cv.MAX_IDS, cv.MAX_QUERIES, cv.MAX_LOCAL, cv.MAX_KF, cv.MAX_CAP) == (65536, 64, 256, 4096, 4096)
    assert (int(got["AFV_COVIS_QUERY_SLOT"]), int(got["AFV_COVIS_QUERY_IDS"])) == (cv.QUERY_SLOT, cv.QUERY_IDS)
    assert int(got["AFV_ABI_VERSION"]) == 6


def test_refusals_that_need_no_table(afv):
    cv = afv.covisibility
    lib = cv.bind()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    EINVAL = afv._lib.EINVAL
    one = np.zeros(4, np.int32)
    votes, order = np.full(4, 77, np.int32), np.full(4, 77, np.int32)
    n_order, best, nz = np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(4, 77, np.int32)
    q = (cv.CovisQuery * 1)()
    q[0].struct_size = C.sizeof(cv.CovisQuery)
    fake = C.c_void_p(0)  # no table: refused before anything is read from it
    outs = (p(votes), p(order), p(n_order), p(best), p(nz))
    assert lib.afv_table_covis_votes(fake, fake, p(one), p(one), None, 1, q, 1, *outs) == EINVAL
    assert lib.afv_table_covis_votes(None, None, None, None, None, 0, None, 0, None, None, None, None, None) == EINVAL
    for a in (votes, order, n_order, best, nz):
        assert (a == 77).all()
    ids, seen = np.full(4, 77, np.int32), np.full(4, 77, np.uint8)
    n = C.c_int32(77)
    assert lib.afv_table_local_points(fake, fake, p(one), 1, None, 0, 4, p(ids), p(seen), C.byref(n)) == EINVAL
    assert lib.afv_table_local_points(None, None, None, 0, None, 0, 0, None, None, None) == EINVAL
    assert (ids == 77).all() and (seen == 77).all() and n.value == 77

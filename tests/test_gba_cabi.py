"""CPU: the library exports afv_table_global_bundle_adjust and afv_points_correct_se3 (include/afv_hip.h, "Global bundle adjustment"),
_lib.py binds them, the caps are the header's, the records are afv_table_bundle_adjust's at their pinned sizes, the package exports
GlobalBundleAdjustment and MapPoints.correct_se3, every refusal that needs no table answers AFV_EINVAL with the poisoned outputs
untouched (the refusals that need a table and a store are in tests/test_gpu_gba.py), the plan's capacity answer is AFV_ECAPACITY without
a device, afv_table_bundle_adjust still refuses 65 free keyframes, and the ABI revision is still 6."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound(afv):
    lib = afv._lib.load()
    for name, nargs in (("afv_table_global_bundle_adjust", 18), ("afv_points_correct_se3", 8), ("afv_gba_plan_probe", 7)):
        assert hasattr(lib, name) and name in afv._lib.SYMBOLS
        assert getattr(lib, name).argtypes == afv._lib.SYMBOLS[name][1] and len(afv._lib.SYMBOLS[name][1]) == nargs
    assert afv._lib.SYMBOLS["afv_table_global_bundle_adjust"][1] == afv._lib.SYMBOLS["afv_table_bundle_adjust"][1]
    assert lib.afv_abi_version() == 6 and afv._lib.ABI_VERSION == 6
    assert afv.GlobalBundleAdjustment is afv.lba.GlobalBundleAdjustment and hasattr(afv.MapPoints, "correct_se3")


def test_caps_and_records_match_the_header(afv, tmp_path):
    L = afv._lib
    src = tmp_path / "caps.c"
    src.write_text('#include <stdio.h>\n#include "afv_hip.h"\nint main(void) {\n'
                   '  printf("%d %d %d %d\\n", AFV_GBA_MAX_KF, AFV_GBA_MAX_POINTS, AFV_GBA_MAX_EDGES, AFV_GBA_MAX_L_BLOCKS);\n'
                   '  printf("%d %d %d %d %d\\n", AFV_LBA_MAX_FREE, AFV_ESS_MAX_KF, AFV_ABI_VERSION, AFV_POINT_MOVED, AFV_POINT_NO_PAIR);\n'
                   '  printf("%zu %zu %zu\\n", sizeof(afv_lba_cam), sizeof(afv_lba_params), sizeof(afv_lba_result));\n  return 0;\n}\n')
    exe = tmp_path / "caps"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines()]
    assert out[0] == [L.GBA_MAX_KF, L.GBA_MAX_POINTS, L.GBA_MAX_EDGES, L.GBA_MAX_L_BLOCKS] == [4096, 524288, 2097152, 1048576]
    assert out[1] == [64, L.GBA_MAX_KF, 6, L.POINT_MOVED, L.POINT_NO_PAIR]
    assert out[2] == [C.sizeof(L.LbaCam), C.sizeof(L.LbaParams), C.sizeof(L.LbaResult)] == [72, 32, 64]


def _call(afv, entry, **over):
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
    a = dict(t=None, pts=None, slots=ints, nk=2, nf=1, cams=cams, ids=ints, npts=2, op=ints, ok=ints, oi=ints, ne=2, prm=prm, res=res, kf=kf, xyz=xyz,
             state=state)
    a.update(over)
    p = lambda v: L.ptr(v) if isinstance(v, np.ndarray) else v
    code = getattr(lib, entry)(a["t"], a["pts"], p(a["slots"]), a["nk"], a["nf"], a["cams"], p(a["ids"]), a["npts"], p(a["op"]), p(a["ok"]), p(a["oi"]),
                               a["ne"], None if a["prm"] is None else C.byref(a["prm"]), None, None if a["res"] is None else C.byref(a["res"]),
                               p(a["kf"]), p(a["xyz"]), p(a["state"]))
    untouched = bytes(res) == b"\xa5" * C.sizeof(res) and np.all(kf == 7.5) and np.all(xyz == 7.5) and np.all(state == 0xA5)
    return code, untouched


def test_refusals_without_a_table_leave_the_outputs_untouched(afv):
    L = afv._lib
    entry = "afv_table_global_bundle_adjust"
    assert _call(afv, entry) == (L.EINVAL, True)
    for bad in (dict(slots=None), dict(cams=None), dict(ids=None), dict(op=None), dict(ok=None), dict(oi=None), dict(prm=None), dict(res=None),
                dict(kf=None), dict(xyz=None), dict(state=None), dict(nk=L.GBA_MAX_KF + 1), dict(nk=L.GBA_MAX_KF + 1, nf=L.GBA_MAX_KF + 1), dict(nf=3),
                dict(nk=-1), dict(nf=-1), dict(npts=L.GBA_MAX_POINTS + 1), dict(ne=L.GBA_MAX_EDGES + 1), dict(ne=-1), dict(npts=-1)):
        assert _call(afv, entry, **bad) == (L.EINVAL, True), bad


def test_the_old_entry_point_keeps_its_cap_of_64_free_keyframes(afv):
    L = afv._lib
    assert L.LBA_MAX_FREE == 64
    assert _call(afv, "afv_table_bundle_adjust", nk=66, nf=65) == (L.EINVAL, True)
    assert _call(afv, "afv_table_bundle_adjust", nk=L.LBA_MAX_KF + 1, nf=1) == (L.EINVAL, True)


def test_correct_se3_refusals_without_a_store(afv):
    L = afv._lib
    lib = L.load()
    ids, T, st = np.zeros(4, np.int32), np.zeros(24, np.float32), np.full(4, 0xA5, np.uint8)
    assert lib.afv_points_correct_se3(None, L.ptr(ids), 1, L.ptr(ids), L.ptr(T), L.ptr(T), 1, L.ptr(st)) == L.EINVAL
    assert np.all(st == 0xA5)


def test_the_plan_answers_ecapacity_without_a_device(afv):
    """one point seen by nf keyframes makes every pair structural: nf (nf + 1) / 2 blocks.  The probe takes the block cap as an argument
    (the entry point always uses AFV_GBA_MAX_L_BLOCKS); at that cap, 1448 keyframes are one too many"""
    L = afv._lib
    lib = L.load()
    counts = np.full(3, -7, np.int32)

    def probe(nf, cap):
        op, ok = np.zeros(nf, np.int32), np.arange(nf, dtype=np.int32)
        return lib.afv_gba_plan_probe(nf, 1, L.ptr(op), L.ptr(ok), nf, cap, L.ptr(counts))

    assert probe(10, 55) == 0 and list(counts) == [55, 55, 10]
    counts[:] = -7
    assert probe(10, 54) == L.ECAPACITY and np.all(counts == -7)
    assert probe(1447, L.GBA_MAX_L_BLOCKS) == 0 and counts[0] == 1447 * 1448 // 2 <= L.GBA_MAX_L_BLOCKS
    counts[:] = -7
    assert probe(1448, L.GBA_MAX_L_BLOCKS) == L.ECAPACITY and np.all(counts == -7)

"""CPU: tools/essgraph_host.cpp, the scalar host program that tools/time_essgraph.py times and compares the device with, answers what the
restatement tests/_essgraph_ref.py answers, bit for bit, on every constructed scene: the estimates, the poses, the inverses, the counts
and the trace; its plan (csrc/afv_essgraph_plan.h, the one the library builds) counts the blocks of L the restatement's symbolic
factorisation counts, and refuses what exceeds the caps.  The same source, built as the stand-alone program it also is with
-fsanitize=address,undefined, runs clean on every scene (no sanitizer touches code loaded into Python)."""
import subprocess

import numpy as np
import pytest

import _essgraph_host as H
import _essgraph_ref as G
import _essgraph_scenes as SC


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return H.build_host(tmp_path_factory.mktemp("essgraph_host") / "essgraph_host.so")


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_host_program_is_bit_equal_to_the_restatement(host_program, name):
    sc, pr, want, _ = SC.solved(name)
    got = H.run_host(host_program, sc)
    assert got.plan == 0
    assert (got.iterations, got.trials, got.l_blocks, got.status, got.n_updates) == (want.iterations, want.trials, pr.l_blocks, want.status, pr.n_updates), name
    assert np.array([got.chi2_first, got.chi2_last, got.lam]).tobytes() == np.array([want.chi2_first, want.chi2_last, want.lam], np.float64).tobytes(), name
    assert got.S.tobytes() == H.records(want.S).tobytes(), name
    assert got.Tiw.tobytes() == want.Tiw.tobytes(), name
    assert got.Swc.tobytes() == H.records(want.Swc).tobytes(), name


def test_point_correction_is_bit_equal_to_the_restatement(host_program):
    sc, pr, want, _ = SC.solved("drifted_loop")
    pos, flags, ids, ref = SC.points_for(sc)
    pos_ref, pos_host = pos.copy(), pos.copy()
    xyz, st = G.correct_points(pos_ref, flags, ids, ref, sc["S_init"], want.Swc)
    gx, gs = H.host_correct(host_program, pos_host, flags, ids, ref, H.records(sc["S_init"]), H.records(want.Swc))
    assert np.array_equal(gs, st) and set(st) == {G.MOVED, G.BAD_OR_UNSET, G.NO_PAIR}
    assert gx.tobytes() == xyz.tobytes() and pos_host.tobytes() == pos_ref.tobytes()
    assert not np.array_equal(pos_ref, pos)


def test_plan_refuses_a_fill_beyond_the_caps(host_program):
    # vertex 1 is joined with every later vertex: eliminating it first fills the whole lower triangle
    n = 40
    I = (np.eye(3), np.zeros(3), 1.0)
    sc = SC.scene([I] * n, 0, [(k, 1) for k in range(2, n)], [I] * n)
    full = (n - 1) * n // 2
    assert H.run_host(host_program, sc).l_blocks == full == SC.problem(sc).l_blocks
    assert H.run_host(host_program, sc, max_blocks=full - 1).plan == 1
    assert H.run_host(host_program, sc, max_updates=10).plan == 2


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "essgraph_host"
    r = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DESSGRAPH_HOST_MAIN", "-I", H.INC, H.SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for name in sorted(SC.SCENES):
        sc, pr, want, _ = SC.solved(name)
        pos, flags, ids, ref = SC.points_for(sc)
        ok = ((flags[ids] & G.SET) != 0) & ((flags[ids] & G.BAD) == 0)
        H.write_scene_file(tmp_path / "scene.bin", sc, pos[ids], ok, ref)
        r = subprocess.run([str(exe), str(tmp_path / "scene.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        assert "plan 0 iterations %d trials %d l_blocks %d updates %d status %d " % (want.iterations, want.trials, pr.l_blocks, pr.n_updates, want.status) in r.stdout, (name, r.stdout)
    r = subprocess.run([str(exe), str(tmp_path / "scene.bin"), "0"], capture_output=True, text=True, timeout=120)   # the refusal path
    assert r.returncode == 0 and "plan 1 " in r.stdout, (r.stdout, r.stderr)

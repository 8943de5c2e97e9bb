"""-m gpu: afv::OptimizeEssentialGraph and afv::CorrectPointsSim3 of adapter/afv_adapter.hpp as a plain C++ process
(adapter/essgraph_selftest): a constructed scene goes in as the scene file of tools/essgraph_host.cpp; the trace, the estimates, the poses,
the corrected points, their statuses and the store's positions come out and equal the restatement's dump (tests/_essgraph_ref.py), bit
for bit, through both entries."""
import os
import subprocess

import numpy as np
import pytest

import _essgraph_host as H
import _essgraph_ref as G
import _essgraph_scenes as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "essgraph_selftest")


@pytest.mark.parametrize("name", ["drifted_loop", "fix_scale_on", "floating"])
def test_cpp_adapter_answers_as_the_restatement(tmp_path, name):
    assert os.path.exists(BIN), "essgraph_selftest is not built: __graft_entry__.build() compiles it"
    sc, pr, want, _ = SC.solved(name)
    npts = 70
    pos, flags, ids, ref = SC.points_for(sc, n=npts, cap=npts, seed=3)
    packed, pflags = pos[ids], flags[ids]
    pflags[pflags == 0] = G.SET | G.BAD                    # the selftest knows bad points only: an unset one travels as a bad one
    ok = (pflags & G.BAD) == 0
    inp, out = tmp_path / "scene.bin", tmp_path / "answer.bin"
    H.write_scene_file(inp, sc, packed, ok, ref)
    r = subprocess.run([BIN, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    nk = pr.nk
    at = 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        return a

    ints, d = take(np.int32, 4), take(np.float64, 3)
    S_out, Tiw, xyz, after, st = take(np.float64, nk * 13), take(np.float64, nk * 12), take(np.float64, npts * 3), take(np.float32, npts * 3), take(np.uint8, npts)
    st2, after2 = take(np.uint8, npts), take(np.float32, npts * 3)
    assert at == len(raw)
    assert list(ints) == [want.iterations, want.trials, pr.l_blocks, want.status]
    assert d.tobytes() == np.array([want.chi2_first, want.chi2_last, want.lam], np.float64).tobytes()
    assert S_out.tobytes() == H.records(want.S).tobytes() and Tiw.tobytes() == want.Tiw.tobytes()
    store = packed.copy()
    wx, ws = G.correct_points(store, pflags, np.arange(npts), ref, sc["S_init"], want.Swc)
    assert np.array_equal(st, ws) and np.array_equal(st2, ws) and set(ws) == {G.MOVED, G.BAD_OR_UNSET, G.NO_PAIR}
    assert xyz.tobytes() == wx.tobytes() and after.tobytes() == store.tobytes() and after2.tobytes() == store.tobytes()

"""-m gpu: afv::PnPsolver of adapter/afv_adapter.hpp as a plain C++ process (adapter/pnp_selftest): one constructed scene of a frame, a
store and four candidates (two of them false) goes in as a file, the trace of Relocalization's iterate(5) loop comes out and is held to the
sequential loop of the restatement (tests/_pnp_ref.py) on the same scene."""
import os
import subprocess

import numpy as np
import pytest

import _pnp_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "pnp_selftest")


def _hx(v):
    return float(np.float32(v)).hex()


def test_cpp_adapter_iterates_as_the_restatement(afv, gpu_ctx, tmp_path):
    assert os.path.exists(BIN), "pnp_selftest is not built: __graft_entry__.build() compiles it"
    s = S.build("adapter", 60, 45, 15, 61, nc=4, false_rows=(1, 3), bad=2, unset=2, octaves=True, min_inliers=10, epsilon=0.5, nhyp=35)
    Rc, tc = s.Rcw.astype(np.float32), s.tcw.astype(np.float32)
    Ow = np.array([-Rc[0, k] * tc[0] + (-Rc[1, k] * tc[1] + -Rc[2, k] * tc[2]) for k in range(3)], np.float32)
    lines = ["%d %d %d %d %d %d %d" % (s.N, s.nc, len(s.store_flags), s.seed, s.nhyp, s.min_inliers, s.nhyp),
             " ".join(_hx(v) for v in (s.epsilon, s.th2, S.W, S.H)), " ".join(_hx(v) for v in list(Rc.ravel()) + list(tc) + list(Ow) + list(s.cam))]
    lines += ["%s %s %d" % (_hx(s.x[i]), _hx(s.y[i]), s.octave[i]) for i in range(s.N)]
    lines += [" ".join(str(v) for v in row) for row in s.rows]
    lines += ["%s %s %s %d" % (_hx(p[0]), _hx(p[1]), _hx(p[2]), f) for p, f in zip(s.store_pos, s.store_flags)]
    inp = tmp_path / "scene.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    kps = np.zeros(s.N, afv.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = s.x, s.y, s.octave
    sigma2 = gpu_ctx.size_sigma(kps)[1]
    want, found_any, exhausted_any = [], False, False
    for c in range(s.nc):
        ref, out = s.solver(c, sigma2), s.run(c, sigma2)
        while True:
            T, no_more, vb, n_in = ref.iterate(5)
            # the record the best set comes from: the one hypothesis so far that is a record and counts mnBestInliers
            hits = np.flatnonzero((out["count"][:ref.mnIterations] == ref.mnBestInliers) & (out["refined"][:ref.mnIterations] != 0))
            best = int(hits[0]) if len(hits) and ref.mnBestInliers else -1
            want.append("%d %d %d %d %d %d %d" % (c, ref.mnIterations, int(no_more), n_in, ref.mnBestInliers, best, int(T is not None)))
            if T is not None:
                found_any = True
                want.append("T " + " ".join(_hx(v) for v in T.ravel()))
                want.append(("i " + " ".join(str(i) for i in np.nonzero(vb)[0])).rstrip())
            if T is not None or no_more:
                exhausted_any = exhausted_any or T is None
                break
    assert found_any and exhausted_any
    got = [l.rstrip() for l in r.stdout.splitlines()]
    tokens = lambda lines: [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in lines for v in l.split()]
    assert tokens(got) == tokens(want)
    assert len(got) == len(want)

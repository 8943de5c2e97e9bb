"""-m gpu: afv::NewMapPoints of adapter/afv_adapter.hpp as a plain C++ process (adapter/newpoints_selftest): a seeded world of a current
keyframe and three neighbours goes in as a file, the created points come out and are held to the composed restatement
(tests/_tri_ref.py with tests/_bow_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import _tri_ref as R
import _tri_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "newpoints_selftest")
FIELDS = ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma")


def _hx(v):
    return float(np.float32(v)).hex()


def test_cpp_adapter_creates_the_restatements_points(afv, gpu_ctx, tmp_path):
    assert os.path.exists(BIN), "newpoints_selftest is not built: __graft_entry__.build() compiles it"
    W = S.World(2, nn=3, n=40)
    none = [np.zeros(W.n, np.uint8) for _ in range(W.nn)]
    want = R.create_new_map_points(W.kfs[0], W.kfs[1:], W.jobs, W.search(60.0), np.zeros(W.n, np.uint8), none, first_id=3)
    lines = ["64 %d %d 3 128 %s" % (W.nn + 1, W.n, _hx(60.0))]
    for kf, d in zip(W.kfs, W.desc):
        for i in range(kf.n):
            lines.append(" ".join([_hx(kf.x[i]), _hx(kf.y[i]), _hx(kf.sigma2[i]), _hx(kf.size[i])] + [str(int(b)) for b in d[i]]))
    for k, j in enumerate(W.jobs):
        vals = list(j.Rcw1) + list(j.tcw1) + list(j.Ow1) + list(j.Rcw2) + list(j.tcw2) + list(j.Ow2) + [getattr(j, f) for f in R.Job.FIELDS]
        assert len(vals) == 47
        lines.append(" ".join(_hx(v) for v in vals))
        lines.append(" ".join(_hx(v) for v in list(W.F12[k]) + list(W.epipoles[k])))
    inp = tmp_path / "world.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    made = [tuple(int(v) for v in l.split()) for l in out if not l.startswith("p ")]
    assert made == [(nid, 0, i, k + 1, j) for nid, k, i, j, _ in want] and len(made) > W.n // 2
    stored = {int(l.split()[1]): l.split()[2:] for l in out if l.startswith("p ")}
    for nid, _, _, _, f in want:
        vals = np.array([float.fromhex(v) for v in stored[nid][:11]], np.float32)
        ref = np.concatenate([np.ravel(f[k]) for k in FIELDS]).astype(np.float32)
        assert vals.view(np.uint32).tolist() == ref.view(np.uint32).tolist(), nid
        assert int(stored[nid][11]) == 5

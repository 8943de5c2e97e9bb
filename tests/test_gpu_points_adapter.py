"""-m gpu: afv::DeviceMapPoints and DeviceFrame::SearchLocalPoints / SearchByProjectionLast / SearchByProjectionReloc / FusePoints of
adapter/afv_adapter.hpp as a plain C++ process (adapter/points_selftest): a seeded random scene goes in as a file, the four answers come
out and are held to the restatement (tests/_points_ref.py composed with tests/_proj_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import _points_ref as R
import _points_scenes as S
import _proj_ref as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "points_selftest")


def _hx(v):
    return float(np.float32(v)).hex()


def test_cpp_adapter_point_searches(afv, gpu_ctx, tmp_path):
    assert os.path.exists(BIN), "points_selftest is not built: __graft_entry__.build() compiles it"
    s = S.random_scene(1, R.LASTFRAME)
    P, cam, f = s.P, s.cam, s.feat
    ids = np.flatnonzero(P.flags & R.SET)
    lines = ["%d %d" % (P.capacity, len(ids))]
    for i in ids:
        vals = list(P.pos[i]) + list(P.normal[i]) + [P.min_distance[i], P.max_distance[i], P.ref_size[i], P.ref_distance[i], P.ref_sigma[i]]
        lines.append(" ".join([str(i)] + [_hx(v) for v in vals] + [str(int(bool(P.flags[i] & R.BAD))), str(int(bool(P.flags[i] & R.OBSERVED)))] +
                              [str(int(b)) for b in P.descriptors[i]]))
    pose = list(cam.Rcw.reshape(9)) + list(cam.tcw) + list(cam.Ow) + [cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf]
    lines.append(" ".join(_hx(v) for v in pose))
    lines.append("%s %s %d" % (_hx(S.W), _hx(S.H), f.n))
    for k in range(f.n):
        lines.append(" ".join([_hx(f.x[k]), _hx(f.y[k]), _hx(f.sizes[k]), _hx(f.angles[k])] + [str(int(b)) for b in f.desc[k]]))
    lines.append(str(len(s.ids)))
    for k in range(len(s.ids)):
        lines.append("%s %s" % (_hx(s.last_sizes[k]), _hx(s.last_angles[k])))
    lines.append(str(len(s.ids)))
    lines.append(" ".join(str(int(i)) for i in s.ids))
    lines.append(" ".join(_hx(v) for v in (s.radius_th, s.cos_limit, s.th, s.nnratio)))
    inp = tmp_path / "scene.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {}
    for l in r.stdout.splitlines():
        head, _, body = l.partition(":")
        got[head.split()[0]] = (int(head.split()[1]) if " " in head else None, np.array(body.split(), np.int64))

    def scene(flavour):
        last = flavour == R.LASTFRAME
        return S.Scene(s.name, None, flavour, P, cam, s.ids, None, radius_th=s.radius_th, cos_limit=s.cos_limit,
                       last_sizes=s.last_sizes if last else None, last_angles=None if flavour in (R.FRUSTUM, R.FUSE) else s.last_angles, feat=f,
                       th=s.th, nnratio=s.nnratio, check_orientation=flavour in (R.LASTFRAME, R.RELOC))

    for tag, flavour in (("local", R.FRUSTUM), ("last", R.LASTFRAME), ("reloc", R.RELOC), ("fuse", R.FUSE)):
        want, wn, o = S.expected_search(afv, PR, scene(flavour))
        assert got[tag][0] == wn and np.array_equal(got[tag][1], want), tag
        assert wn >= 5, tag
        if tag == "local":
            assert np.array_equal(got["inview"][1] != 0, o["in_view"])

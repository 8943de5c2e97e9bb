"""-m gpu: afv::Initializer of adapter/afv_adapter.hpp as a plain C++ process (adapter/init_selftest): a constructed scene goes in as a
file, what Initialize returns (and the trace's counts and cosines) comes out and is held to the restatement tests/_init_ref.py, bit for
bit.  One scene that ReconstructF accepts, one that ReconstructH accepts."""
import os
import subprocess

import numpy as np
import pytest

import _init_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "init_selftest")


def _hx(v):
    return float(np.float32(v)).hex()


def _tokens(lines):
    return [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in lines for v in l.split()]


@pytest.mark.parametrize("name", ["cloud", "plane"])
def test_cpp_adapter_answers_as_the_restatement(name, tmp_path):
    assert os.path.exists(BIN), "init_selftest is not built: __graft_entry__.build() compiles it"
    sc, want = S.scene(name), S.reference(name)
    tr = want["trace"]
    lines = ["%d %d %d %d" % (len(sc.x1), len(sc.x2), sc.iterations, sc.seed), " ".join(_hx(v) for v in (sc.fx, sc.fy, sc.cx, sc.cy, sc.sigma))]
    lines += ["%s %s %d" % (_hx(x), _hx(y), m) for x, y, m in zip(sc.x1, sc.y1, sc.matches12)]
    lines += ["%s %s" % (_hx(x), _hx(y)) for x, y in zip(sc.x2, sc.y2)]
    inp = tmp_path / "scene.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert want["ok"] == 1
    exp = ["%d %d %d %d %d %d %d %d" % (want["ok"], want["route"], tr["reason"], tr["N"], tr["best"][0], tr["best"][1], tr["n_motion"],
                                        tr["best_motion"]),
           "R " + " ".join(_hx(v) for v in want["R21"]), "t " + " ".join(_hx(v) for v in want["t21"])]
    exp += ["m %d %s" % (c["n_good"], _hx(c["cos"])) for c in tr["checks"]]
    exp += ["p %d %s %s %s" % (g, _hx(p[0]), _hx(p[1]), _hx(p[2])) for g, p in zip(want["triangulated"], want["p3d"])]
    got = [l.rstrip() for l in r.stdout.splitlines()]
    assert len(got) == len(exp)
    assert _tokens(got) == _tokens(exp)

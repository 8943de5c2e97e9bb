"""-m gpu: afv::CovisibilityVotes, afv::LocalPoints and afv::CovisibilityGraph of the C++ adapter (adapter/covis_selftest) as a plain C++
process on the scenes of tests/_covis_scenes.py: the two calls against the restatement, the graph and its local map against the Python mirror
run over the restatement (a stand-in for the device, tests/test_covis_ref_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import _covis_ref as R
import _covis_scenes as S
from test_covis_ref_cpu import _stand_ins

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anyfeature-vslam_amd", "adapter", "covis_selftest")


def _lst(v):
    v = [int(x) for x in v]
    return " ".join(str(x) for x in [len(v)] + v)


def scene_text(sc, th):
    lines = ["%d %d %d %d" % (sc["nsets"], sc["cap"], sc["capacity"], th)]
    lines += [_lst(sc["planes"].get(s, [])) for s in range(sc["nsets"])]
    lines += [_lst(sc["set"]), _lst(sc["bad"]), str(len(sc["slots"]))]
    bad = sc["kf_bad"] or [0] * len(sc["slots"])
    lines += ["%d %d %d" % (s, k, b) for s, k, b in zip(sc["slots"], sc["key_ids"], bad)]
    lines.append(str(len(sc["queries"])))
    for q in sc["queries"]:
        lines.append("%d %d %d %d %s" % (0 if "slot" in q else 1, q.get("slot", -1), q.get("th", 15), int(q.get("skip_bad", False)), _lst(q.get("ids", []))))
    lines += [_lst(sc["local"] or []), _lst(sc["frame_pts"] or [])]
    return "\n".join(lines) + "\n"


def expected(afv, sc, th):
    ln = lambda tag, v: (tag + " " + " ".join(str(int(x)) for x in v)).rstrip()
    a = S.answer(sc)
    out = []
    for q in range(len(sc["queries"])):
        out += ["Q %d %d" % (a["best"][q], a["nz"][q]), ln("V", a["votes"][q]), ln("O", a["order"][q])]
    out += [ln("L", a.get("local_ids", [])), ln("S", a.get("seen", []))]

    class _T:
        nsets, cap = sc["nsets"], sc["cap"]
    g = afv.CovisibilityGraph(_T(), None, *_stand_ins(sc["planes"], R.Store(sc["capacity"], sc["set"], sc["bad"])))
    g.TH = th
    bad = sc["kf_bad"] or [0] * len(sc["slots"])
    for s, k, b in zip(sc["slots"], sc["key_ids"], bad):
        g.add_keyframe(s, k)
        if b:
            g.set_bad(s)
    g.UpdateConnectionsBatch(sc["slots"])
    for s in sc["slots"]:
        p = g.GetParent(s)
        out += ["G %d %d" % (s, -1 if p is None else p), ln("C", g.GetVectorCovisibleKeyFrames(s)), ln("W", g.kf[s].ordered_w), ln("N", g.GetConnectedKeyFrames(s))]
    d = g.essential_graph_dict(min_feat=th)
    for key in sorted(d["parent"]):
        out += ["E %d %d" % (key, -1 if d["parent"][key] is None else d["parent"][key]), ln("EC", d["covisibles"][key])]
    if sc["slots"]:
        out += [ln("B", g.best_covisibles(sc["slots"][0])), ln("D", g.connected(sc["slots"][0]))]
    m = g.UpdateLocalMap(sc["frame_pts"] or [], 80, 10)
    if m is None:
        out += ["M 0 -1", "K", "L", "S"]
    else:
        out += ["M 1 %d" % (-1 if m[1] is None else m[1]), ln("K", m[0]), ln("L", m[2]), ln("S", m[3])]
    return out, g


SCENES = [(S.order_ties, 15), (S.best_tie, 15), (S.skip_bad, 1), (S.good_filter, 1), (S.first_occurrence, 1), (S.plane_duplicate, 1),
          (lambda: S.random_scene(51, counts=[60, 0, 64, 65, 33, 50, 1, 40, 64, 20], cap=65, capacity=300, nq_slot=10, id_lengths=(80, 0, 300), th=4,
                                  with_bad_kf=True, local=[8, 2, 0, 5], n_frame=60, pool=120), 4),
          (lambda: S.random_scene(52, counts=[30] * 70, cap=32, capacity=400, nq_slot=64, id_lengths=(), th=3, local=list(range(0, 70, 2)), n_frame=90,
                                  pool=150), 3)]


@pytest.mark.parametrize("case", range(len(SCENES)))
def test_cpp_adapter_answers_as_the_restatement(afv, gpu_ctx, tmp_path, case):
    assert os.path.exists(EXE), "covis_selftest is not built: __graft_entry__.build() compiles it"
    make, th = SCENES[case]
    sc = make()
    want, g = expected(afv, sc, th)
    if case >= 6:
        assert any(len(g.kf[s].ordered) > 1 for s in sc["slots"]) and any(g.kf[s].parent is not None for s in sc["slots"])
    inp = tmp_path / "scene.txt"
    inp.write_text(scene_text(sc, th))
    r = subprocess.run([EXE, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [l.rstrip() for l in r.stdout.splitlines()] == want

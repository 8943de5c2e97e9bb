"""CPU: the oracle's float32 AKAZE61 chain (oracle/akaze.c) against the float64 restatement of tests/_akaze_f64.py, on the edge scenes and
on seeded synth frames: FED steps, kcontrast, and every plane of every level within the committed bounds."""
import importlib

import numpy as np
import pytest

import _akaze_f64 as F
import _akaze_scenes as SC

synth = importlib.import_module("anyfeature-vslam_amd.synth")

FRAMES = [(n, None) for n in SC.NAMES] + [("synth", (1, 206, 110)), ("synth", (2, 320, 240)), ("synth", (3, 640, 480)), ("synth", (4, 111, 65))]


def _frame(name, arg):
    return SC.scene(name) if arg is None else synth.corners_frame(arg[0], arg[1], arg[2])


@pytest.fixture(scope="module")
def akz():
    from oracle import akaze_binding
    return akaze_binding


def test_fed_steps_closed_form(akz):
    for (w, h) in ((1280, 720), (206, 110)):
        p = akz.make_plan(w, h)
        for i in range(1, p.nlevels):
            T = float(p.lv[i].etime) - float(p.lv[i - 1].etime)
            t64 = F.fed_tau(T)
            t32 = np.array(list(p.lv[i].tau)[:p.lv[i].nsteps], np.float64)
            assert len(t64) == len(t32) == p.lv[i].nsteps
            assert np.max(np.abs(t32 - t64) / t64) <= F.BOUND_TAU, (i, t32, t64)
            assert abs(t64.sum() - T) < 1e-9 * max(T, 1)        # a cycle covers exactly its evolution time
            assert t64.max() > 0.25                              # FED: single steps beyond the explicit stability limit


def test_gaussian_taps_match(akz):
    p = akz.make_plan(320, 240)
    for sigma, taps, n in ((1.6, p.gauss_soffset, p.ksize_soffset), (1.0, p.gauss_one, p.ksize_one)):
        t = F.gauss_taps(sigma)
        assert len(t) == n and np.max(np.abs(np.array(list(taps)[:n]) - t)) < 1e-7


@pytest.mark.parametrize("name,arg", FRAMES, ids=[n if a is None else "synth%dx%d" % a[1:] for n, a in FRAMES])
def test_oracle_planes_within_float64_bounds(akz, name, arg):
    f = _frame(name, arg)
    h, w = f.shape
    p = akz.make_plan(w, h)
    lv, k0 = akz.full_evolution(f, p)
    err = F.check_against_f64(f, p, lv, k0)
    print(name, arg, {k: "%.2g" % max(v) for k, v in err.items()})


def test_kcontrast_bins(akz):
    """the oracle's contrast factor sits in the float64 bin; a neighbouring bin is allowed only where a magnitude lies within the bound of a
    bin boundary, and that must stay rare"""
    neighbours = 0
    for name, arg in FRAMES:
        f = _frame(name, arg)
        h, w = f.shape
        _, k0 = akz.scale_space(f, akz.make_plan(w, h))
        ok, k64, nb = F.kcontrast_bin_ok(f, k0)
        assert ok, (name, arg, k0, k64)
        neighbours += nb
    print("kcontrast: %d of %d frames needed the neighbouring bin" % (neighbours, len(FRAMES)))
    assert neighbours <= 1


def test_restatement_is_not_the_oracle(akz):
    """sanity of the yardstick: the float64 chain differs from the float32 one (it is not a copy), but only by rounding"""
    f = synth.corners_frame(5, 206, 110)
    p = akz.make_plan(206, 110)
    lv, k0 = akz.full_evolution(f, p)
    ref = F.scale_space(f, p, k0=np.float32(k0))
    err = F.plane_errors(lv, ref)
    assert max(err["Lt"]) > 0 and max(err["Ldet"]) > 0
    # a wrong FED step (one tau off by 1 %) is far outside the bound
    bad = [dict(d) for d in lv]
    L = p.lv[3]
    tau = F.fed_tau(L.etime - p.lv[2].etime)
    lt = ref[2]["Lt"]
    c = F.conductivity(F.gauss(lt, 1.0), float(np.float32(k0)))
    for j, t in enumerate(tau):
        lt = F.nld_step(lt, c, t * (1.01 if j == 0 else 1.0))
    bad[3]["Lt"] = lt.astype(np.float32)
    assert F.plane_errors(bad, ref)["Lt"][3] > F.BOUND_PLANE["Lt"]


@pytest.mark.parametrize("name,arg", FRAMES[:-2] + FRAMES[-1:], ids=[n if a is None else "synth%dx%d" % a[1:] for n, a in FRAMES[:-2] + FRAMES[-1:]])
def test_oracle_detection_and_descriptors_against_float64(akz, name, arg):
    """candidates, the subpixel step, the orientation and the MLDB bits of the oracle against the float64 restatement, wherever the float64
    margin exceeds the bound; the excluded items are counted, reported and bounded"""
    f = _frame(name, arg)
    h, w = f.shape
    p = akz.make_plan(w, h)
    lv, k0 = akz.full_evolution(f, p)
    ref = F.scale_space(f, p, k0=np.float32(k0))
    cands = [akz.level_candidates(p, i, lv[i]["Ldet"]) for i in range(p.nlevels)]
    un = akz.find_extrema(p, lv)
    re = akz.subpixel(p, lv, un)
    d_cmp, d_exc = F.check_detection_f64(f, p, ref, cands, un, re)
    kp, desc = akz.compute_descriptors(p, lv, re)
    a_cmp, a_exc, a_tie, b_cmp, b_exc = F.check_descriptors_f64(p, ref, kp, desc)
    print("%s: detection %d compared / %d excluded, angles %d / %d (%d ties), MLDB bits %d / %d" % (name, d_cmp, d_exc, a_cmp, a_exc, a_tie,
                                                                                                 b_cmp, b_exc))
    assert d_exc <= 0.02 * max(d_cmp, 1)          # measured: at most 1.5 % (mirror)
    if name == "synth":              # textured frames: few near-ties (the edge scenes are made of them, see tests/_akaze_scenes.py)
        # measured: angles at most 0.1 %, bits at most 10.7 % (111 x 65, five keypoints; 2.8 % at 320 x 240)
        assert a_exc <= 0.02 * max(a_cmp, 1) + 1 and b_exc <= 0.15 * max(b_cmp, 1)
        assert d_cmp > 0 and b_cmp > 0

"""What the Initializer tests share: the comparison of an answer (the device's through afv_frame_initializer, the C++ adapter's, the scalar
host program's) with the restatement's, bit for bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _init_ref as R


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, np.asarray(got).dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = bits(got) != bits(want)
    if got.dtype == np.float32:
        differ &= ~(np.isnan(got) & np.isnan(want))   # a NaN's sign and payload are not pinned (numpy, the host compilers and the device differ)
    if differ.any():
        bad = np.argwhere(differ)
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, want %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])],
                                                                                     want[tuple(bad[0])]))


def check_against(got, want, sc, what):
    """every output of the call against the restatement's answer `want`"""
    tr, t = want["trace"], got["trace"]
    N, it = tr["N"], sc.iterations
    assert (got["ok"], got["route"]) == (want["ok"], want["route"]), what
    for k in ("R21", "t21", "p3d", "triangulated"):
        same(got[k], want[k], what + " " + k)
    assert (t.n, t.best_h, t.best_f, t.route, t.n_inliers, t.n_motion, t.best_motion, t.reason) == (
        N, tr["best"][0], tr["best"][1], want["route"], tr["n_inliers"], tr["n_motion"], tr["best_motion"], tr["reason"]), what
    same(np.array([t.sh, t.sf], np.float32), np.array([tr["SH"], tr["SF"]], np.float32), what + " SH SF")
    same(np.array([t.rh], np.float32), np.array([tr["RH"]], np.float32), what + " RH")
    same(np.array(t.h21, np.float32), tr["model"][0], what + " H21")
    same(np.array(t.f21, np.float32), tr["model"][1], what + " F21")
    same(np.array(t.T1, np.float32), tr["T1"], what + " T1")
    same(np.array(t.T2, np.float32), tr["T2"], what + " T2")
    for i in range(8):
        have = i < tr["n_motion"]
        assert t.n_good[i] == (tr["checks"][i]["n_good"] if have else 0), (what, i)
        same(np.array([t.cos_parallax[i]], np.float32), np.array([tr["checks"][i]["cos"] if have else 0], np.float32), what + " cos %d" % i)
        same(np.array(t.R[i], np.float32), R.flat(tr["motions"][i][0]) if have else np.zeros(9), what + " R %d" % i)
        same(np.array(t.t[i], np.float32), np.array(tr["motions"][i][1], np.float32) if have else np.zeros(3), what + " t %d" % i)
    words = got["inliers"].shape[2]
    for m in range(2):
        hyp = want["hyp"][m]
        same(got["score"][m], [h["score"] for h in hyp] if hyp else np.zeros(it), what + " score %d" % m)
        same(got["degenerate"][m], [h["degenerate"] for h in hyp] if hyp else np.zeros(it), what + " degenerate %d" % m)
        same(got["model"][m], np.stack([h["model"] for h in hyp]) if hyp else np.zeros((it, 9)), what + " model %d" % m)
        same(got["inliers"][m], np.stack([R.mask_words(h["inliers"], words) for h in hyp]) if hyp else np.zeros((it, words)),
             what + " inliers %d" % m)

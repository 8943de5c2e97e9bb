"""Host-side mirror of the reference's Initializer (include/Initializer.h, src/Initializer.cc) as Tracking::MonocularInitialization uses
it (src/Tracking.cc:455, :487): built on the reference frame, asked once per current frame.

Initializer.Initialize makes ONE device call (afv_frame_initializer: the H and F RANSAC over all iterations, the selection, the motion
hypotheses and CheckRT, csrc/k_init.hip) between two resident frames and returns what the reference returns.  Plumbing only: no
arithmetic happens here beyond the display conversion of a cosine to degrees.  The normative semantics, the quirks and the deviations
I1-I11 are tests/_init_ref.py's and include/afv_hip.h's ("Initializer").
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import InitJob, InitTrace, ptr


def initialize(f1, f2, job, matches12, hypotheses=False, mask_words=None, trace=True):
    """afv_frame_initializer as it is.  f1 / f2: resident Frames; job: InitJob; matches12 [N1].  -> dict(ok, route, R21 [9], t21 [3], p3d
    [N1, 3], triangulated [N1], trace (InitTrace | None)), plus score [2, it], model [2, it, 9], degenerate [2, it], inliers [2, it,
    mask_words] when `hypotheses`.  mask_words None: what N1 needs"""
    m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    n1 = f1.N
    if len(m) != n1:
        raise ValueError("Initializer: matches12 has %d entries, the reference frame %d features" % (len(m), n1))
    if mask_words is None:
        mask_words = (n1 + 31) // 32
    mask_words = int(mask_words)
    it = int(job.iterations)
    ok_shape = 1 <= it <= _lib.INIT_MAX_ITERATIONS and 0 <= mask_words <= _lib.INIT_MAX_MASK_WORDS
    h, w = (it, mask_words) if ok_shape else (1, 1)  # an absurd size is the library's to refuse: no array of that size is made for it
    out = dict(R21=np.zeros(9, np.float32), t21=np.zeros(3, np.float32), p3d=np.zeros((n1, 3), np.float32), triangulated=np.zeros(n1, np.uint8),
               trace=_lib.sized(InitTrace) if trace else None)
    if hypotheses:
        out.update(score=np.zeros((2, h), np.float32), model=np.zeros((2, h, 9), np.float32), degenerate=np.zeros((2, h), np.uint8),
                   inliers=np.zeros((2, h, w), np.uint32))
    ok, route = C.c_int32(0), C.c_int32(0)
    f1.ctx.check(f1.lib.afv_frame_initializer(
        f1.handle, f2.handle, C.byref(job), ptr(m), C.byref(ok), C.byref(route), ptr(out["R21"]), ptr(out["t21"]), ptr(out["p3d"]),
        ptr(out["triangulated"]), C.byref(out["trace"]) if trace else None, ptr(out.get("score")), ptr(out.get("model")),
        ptr(out.get("degenerate")), ptr(out.get("inliers")), mask_words), "afv_frame_initializer")
    out.update(ok=int(ok.value), route=int(route.value))
    return out


class Initializer:
    """the reference's interface: Initializer(ReferenceFrame, sigma, iterations) reads K from the frame; here K is handed over
    (a 3 x 3 matrix or (fx, fy, cx, cy))"""

    def __init__(self, ReferenceFrame, K, sigma=1.0, iterations=200):
        self.frame = ReferenceFrame
        K = np.asarray(K, np.float32)
        fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.reshape(4)
        j = _lib.sized(InitJob)
        j.iterations = int(iterations)
        j.fx, j.fy, j.cx, j.cy, j.sigma = float(fx), float(fy), float(cx), float(cy), float(np.float32(sigma))
        self.job = j
        self.trace = None
        self._hyp = None

    def Initialize(self, CurrentFrame, matches12, seed=0, hypotheses=False):
        """-> (ok, R21 [3, 3], t21 [3], vP3D [N1, 3], vbTriangulated [N1] bool).  `hypotheses` keeps the per-hypothesis tables for
        .hypotheses()"""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.job.seed_lo, self.job.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        out = initialize(self.frame, CurrentFrame, self.job, matches12, hypotheses=hypotheses)
        self.trace = out["trace"]
        self.route = out["route"]
        self._hyp = {k: out[k] for k in ("score", "model", "degenerate", "inliers")} if hypotheses else None
        return bool(out["ok"]), out["R21"].reshape(3, 3), out["t21"], out["p3d"], out["triangulated"].astype(bool)

    def hypotheses(self):
        """score [2, iterations], model [2, iterations, 9], degenerate [2, iterations], inliers [2, iterations, mask_words] of the last
        Initialize(..., hypotheses=True); row 0 = homographies, row 1 = fundamental matrices"""
        if self._hyp is None:
            raise RuntimeError("Initializer.hypotheses: call Initialize(..., hypotheses=True) first")
        return self._hyp

    def parallax_degrees(self):
        """the selected cosine of every motion hypothesis of the last call as the reference's parallax in degrees (display only: the
        decisions were taken on the cosines)"""
        t = self.trace
        return [math.degrees(math.acos(max(-1.0, min(1.0, t.cos_parallax[i])))) for i in range(t.n_motion)]

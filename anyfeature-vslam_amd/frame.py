"""Host-side mirror of the reference's Frame as far as the front end goes (include/Frame.h, src/Frame.cc:171-240,333-433): the
device-resident frame of the C-ABI (afv_frame_*).

In the reference a Frame is built once - ExtractFeatures (Frame.cc:242-259), UndistortKeyPoints (:403-433), AssignFeaturesToGrid
(:225-240) - and then read by every matcher of the tracking step.  `Frame` keeps that object on the GPU: `extract` returns the host
vectors the reference's members hold (mvKeys, mDescriptors, keyPtsSigma2 / Inf / Size) AND leaves keypoints, descriptors, the
per-feature scale data and the 64 x 48 grid in HBM; SearchByProjection / Fuse / SearchForInitialization / ComputeBoW /
SearchByBoW(KF, F) / the promotion to a keyframe then run against them without uploading the frame again.
Stereo and RGB-D frames: ComputeStereoMatches (Frame.cc:465-645) between two resident frames that kept their pyramids, and
ComputeStereoFromRGBD (:648-669), fill mvuRight / mvDepth on the device, where the projection searches and the keyframe table read them.
Plumbing only: every method is one C-ABI call.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import KP_DTYPE, FrameParams, ProjQueries, ptr

FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48  # Frame.h:40-41


class Frame:
    def __init__(self, ctx, min_x=0.0, min_y=0.0, max_x=640.0, max_y=480.0, grid_cols=FRAME_GRID_COLS, grid_rows=FRAME_GRID_ROWS,
                 distorted=False, cap=0, desc_bytes=32, float_dim=0, keep_pyramid=False):
        """desc_bytes: size of one binary descriptor (32 ORB, 61 AKAZE, 48 BRISK ...; <= 64); float_dim > 0: float descriptors of that many
        floats instead (SIFT128, SURF64, KAZE64 ...: L2^2 distances) - the reference's matchers dispatch on the descriptor type
        (FeatureMatcher.cc:1508-1531); frames that are not 32-byte binary are filled with set_features.
        keep_pyramid: extract leaves the detector's unblurred pyramid levels with the frame (ComputeStereoMatches reads mvImagePyramid)"""
        self.ctx, self.lib = ctx, ctx.lib
        self.float_dim = int(float_dim)
        self.desc_bytes = 4 * self.float_dim if self.float_dim else int(desc_bytes)
        p = _lib.sized(FrameParams)
        p.min_x, p.min_y, p.max_x, p.max_y = float(min_x), float(min_y), float(max_x), float(max_y)
        p.grid_cols, p.grid_rows, p.distorted, p.cap = int(grid_cols), int(grid_rows), int(bool(distorted)), int(cap)
        p.desc_bytes = int(desc_bytes)
        p.float_dim = self.float_dim
        p.keep_pyramid = int(bool(keep_pyramid))
        self.params = p
        h = C.c_void_p()
        ctx.check(self.lib.afv_frame_create(ctx.handle, C.byref(p), C.byref(h)), "afv_frame_create")
        self.handle = h
        self.sizeTolerance = np.float32(ctx.params.scale_factor)           # Frame.cc:73
        self.invSizeTolerance = np.float32(1.0) / self.sizeTolerance        # Frame.cc:74
        self.grid_inv_w = np.float32(grid_cols) / (np.float32(max_x) - np.float32(min_x))   # Frame.cc:201
        self.grid_inv_h = np.float32(grid_rows) / (np.float32(max_y) - np.float32(min_y))   # Frame.cc:202

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.lib.afv_frame_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def N(self):
        return int(self.lib.afv_frame_count(self.handle))

    # ---- Frame::Frame: extraction into the resident frame ----
    def extract(self, gray, host_outputs=True):
        """FeatureExtractor::operator() (FeatureExtractor.cpp:111-121) into the frame.  Returns (mvKeys, mDescriptors) like
        Context.extract, or N when host_outputs is False (the device copy only)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        self._pyr_sizes = self._level_sizes(w, h) if self.params.keep_pyramid else None
        if not host_outputs:
            self.ctx.check(self.lib.afv_frame_extract(self.handle, ptr(gray), w, h, gray.strides[0], None, None, 0, None), "afv_frame_extract")
            return self.N
        cap = self.ctx.cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int(0)
        self.ctx.check(self.lib.afv_frame_extract(self.handle, ptr(gray), w, h, gray.strides[0], ptr(kps), ptr(desc), cap, C.byref(n)),
                       "afv_frame_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def set_features(self, kps, desc, sizes=None, u_right=None):
        """a frame whose features come from elsewhere (stereo rigs, another extractor, tests): kps (KP_DTYPE), desc [n, desc_bytes]"""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        if self.float_dim:
            desc = np.ascontiguousarray(desc, np.float32).reshape(-1, self.float_dim)
        else:
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, self.desc_bytes)
        sz = None if sizes is None else np.ascontiguousarray(sizes, np.float32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        self.ctx.check(self.lib.afv_frame_set_features(self.handle, ptr(kps), ptr(desc), len(kps), ptr(sz), ptr(ur)), "afv_frame_set_features")

    def set_undistorted(self, x, y):
        """mvKeysUn of a `distorted` frame (cv::undistortPoints is the caller's, Frame.cc:403-433); builds the grid"""
        x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
        self.ctx.check(self.lib.afv_frame_set_undistorted(self.handle, ptr(x), ptr(y)), "afv_frame_set_undistorted")

    # ---- stereo / RGB-D ----
    def _level_sizes(self, w, h):
        """[(lw, lh)] of the context's pyramid for a w x h image"""
        n = C.c_int32(0)
        lw = (C.c_int32 * _lib.MAX_LEVELS)(); lh = (C.c_int32 * _lib.MAX_LEVELS)()
        self.ctx.check(self.lib.afv_pyramid_level_sizes(self.ctx.handle, int(w), int(h), C.byref(n), lw, lh), "afv_pyramid_level_sizes")
        return [(lw[l], lh[l]) for l in range(n.value)]

    def set_pyramid(self, levels):
        """the pyramid of a frame filled with set_features: uint8 [h, w] levels, level 0 the image; the sizes must be the context's
        geometry for that image size (the C side reads exactly those sizes, so they are checked here first)"""
        lv = [np.ascontiguousarray(a, np.uint8) for a in levels]
        if not lv or any(a.ndim != 2 for a in lv):
            raise ValueError("levels: a list of 2-D uint8 images")
        h, w = lv[0].shape
        sizes = self._level_sizes(w, h)
        if len(sizes) != len(lv) or any(a.shape != (lh, lw) for a, (lw, lh) in zip(lv, sizes)):
            raise _lib.AfvError(_lib.EINVAL, "set_pyramid: the levels are not the context's geometry for %d x %d: %r" % (w, h, sizes))
        arr = (C.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        self.ctx.check(self.lib.afv_frame_set_pyramid(self.handle, w, h, arr, len(lv)), "afv_frame_set_pyramid")
        self._pyr_sizes = sizes

    def pyramid(self):
        """the levels the frame holds (keep_pyramid / set_pyramid), back on the host"""
        sizes = getattr(self, "_pyr_sizes", None)
        if sizes is None:
            raise _lib.AfvError(_lib.EINVAL, "the frame holds no pyramid")
        out = []
        for l, (lw, lh) in enumerate(sizes):
            a = np.zeros((lh, lw), np.uint8)
            self.ctx.check(self.lib.afv_frame_get_pyramid_level(self.handle, l, ptr(a)), "afv_frame_get_pyramid_level")
            out.append(a)
        return out

    def ComputeStereoMatches(self, right, mbf, fx, th_high=None, th_low=None):
        """Frame::ComputeStereoMatches (Frame.cc:465-645) of this (left) frame against `right`: fills mvuRight / mvDepth on the device and
        returns the number of features with mvuRight >= 0.  None thresholds = FeatureMatcher.TH_HIGH / TH_LOW.  Semantics:
        tests/_stereo_ref.py (deviations A, B, C of include/afv_hip.h; parity with a build of the reference is unpinned)"""
        from .matcher import FeatureMatcher
        p = _lib.sized(_lib.StereoParams)
        p.mbf, p.fx = float(mbf), float(fx)
        p.th_high = float(FeatureMatcher.TH_HIGH if th_high is None else th_high)
        p.th_low = float(FeatureMatcher.TH_LOW if th_low is None else th_low)
        n = C.c_int32(0)
        self.ctx.check(self.lib.afv_frame_stereo_match(self.handle, right.handle, C.byref(p), C.byref(n)), "afv_frame_stereo_match")
        return int(n.value)

    def ComputeStereoFromRGBD(self, depth, mbf):
        """Frame::ComputeStereoFromRGBD (Frame.cc:648-669): depth = float32 [h, w] image"""
        d = np.asarray(depth, np.float32)
        if d.ndim != 2 or d.strides[1] != 4 or d.strides[0] < 4 * d.shape[1]:   # rows of floats at any row stride are taken as they lie
            d = np.ascontiguousarray(d)
        h, w = d.shape
        self.ctx.check(self.lib.afv_frame_set_depth(self.handle, ptr(d), w, h, d.strides[0], float(mbf)), "afv_frame_set_depth")

    def stereo(self):
        """(mvuRight, mvDepth, sad, best_r): the last two are test outputs of ComputeStereoMatches (-1 where none)"""
        n = self.N
        ur = np.zeros(max(n, 1), np.float32); dp = np.zeros(max(n, 1), np.float32)
        sad = np.zeros(max(n, 1), np.int32); br = np.zeros(max(n, 1), np.int32)
        self.ctx.check(self.lib.afv_frame_get_stereo(self.handle, ptr(ur), ptr(dp), ptr(sad), ptr(br)), "afv_frame_get_stereo")
        return ur[:n], dp[:n], sad[:n], br[:n]

    @property
    def mvuRight(self):
        return self.stereo()[0]

    @property
    def mvDepth(self):
        return self.stereo()[1]

    def grid(self):
        """(cell_ptr[cols * rows + 1], cell_idx[...]) of the device-built grid, cell = ix * rows + iy"""
        nc = self.params.grid_cols * self.params.grid_rows
        cp = np.zeros(nc + 1, np.int32)
        ci = np.zeros(max(self.N, 1), np.int32)
        self.ctx.check(self.lib.afv_frame_get_grid(self.handle, ptr(cp), ptr(ci)), "afv_frame_get_grid")
        return cp, ci[:cp[nc]]

    def device_views(self):
        """raw device pointers (ints): kps, desc, x, y, size, angle, n"""
        out = [C.c_void_p() for _ in range(7)]
        self.ctx.check(self.lib.afv_frame_device_ptrs(self.handle, *[C.byref(o) for o in out]), "afv_frame_device_ptrs")
        return dict(zip(("kps", "desc", "x", "y", "size", "angle", "n"), (o.value for o in out)))

    # ---- Frame::ComputeBoW ----
    def bow_transform_nodes(self, vocabulary, levelsup=4):
        """afv_frame_bow_transform alone: (leaf node, node at depth L - levelsup) per feature; the FeatureVector is built on the device and
        stays with the frame.  ComputeBoW = this + the host-side BowVector / FeatureVector containers"""
        n = self.N
        leaf = np.zeros(max(n, 1), np.int32); nid = np.zeros(max(n, 1), np.int32)
        nn = C.c_int32(0)
        self.ctx.check(self.lib.afv_frame_bow_transform(self.handle, vocabulary._device(), int(levelsup), ptr(leaf), ptr(nid), C.byref(nn)),
                       "afv_frame_bow_transform")
        self._nnodes = int(nn.value)
        return leaf[:n], nid[:n]

    def ComputeBoW(self, vocabulary, levelsup=4):
        """Frame::ComputeBoW (Frame.cc:397-401): returns (BowVector, FeatureVector) like Vocabulary.transform; the FeatureVector also
        stays on the device with the frame"""
        return vocabulary.vectors_from_nodes(*self.bow_transform_nodes(vocabulary, levelsup))

    def bowvec(self):
        """the resident BowVector ComputeBoW / bow_transform_nodes left on the device (a vocabulary with word weights): (word ids
        ascending int32, L1-normalised values float64)"""
        cap = max(self.N, 1)
        word = np.zeros(cap, np.int32); value = np.zeros(cap, np.float64)
        m = C.c_int32(0)
        self.ctx.check(self.lib.afv_frame_get_bowvec(self.handle, ptr(word), ptr(value), C.byref(m)), "afv_frame_get_bowvec")
        return word[:m.value].copy(), value[:m.value].copy()

    def featvec(self):
        """the resident FeatureVector as [(node_id, [feature indices])]"""
        n, nn = self.N, getattr(self, "_nnodes", 0)
        ids = np.zeros(max(nn, 1), np.int32); sp = np.zeros(max(nn, 1) + 1, np.int32); idx = np.zeros(max(n, 1), np.int32)
        self.ctx.check(self.lib.afv_frame_get_featvec(self.handle, ptr(ids), ptr(sp), ptr(idx)), "afv_frame_get_featvec")
        return [(int(ids[k]), idx[sp[k]:sp[k + 1]].tolist()) for k in range(nn)]

    # ---- the projection searches ----
    def _queries(self, q, th, nnratio, mode, check_orientation, occupied=None, qref=None):
        """q: matcher.ProjectionQueries; qref = (DescriptorTable, slots, idx): the queries' descriptors as rows of a keyframe table"""
        s = _lib.sized(ProjQueries)
        keep = []
        s.nq = q.n
        if qref is None:
            if q.n and (q.descriptors.dtype.kind == "f") != bool(self.float_dim):
                raise ValueError("the queries must carry the frame's kind of descriptor")
            s.qdesc = ptr(q.descriptors); s.desc_bytes = q.descriptors.shape[1] * q.descriptors.itemsize if q.n else self.desc_bytes
        else:
            table, slots, idx = qref
            sl = np.ascontiguousarray(slots, np.int32); ix = np.ascontiguousarray(idx, np.int32)
            keep += [sl, ix]
            s.qref_table = table.handle; s.qref_slot = ptr(sl); s.qref_idx = ptr(ix); s.desc_bytes = table.desc_bytes
        s.qvalid = ptr(q.valid); s.qu = ptr(q.u); s.qv = ptr(q.v); s.qr = ptr(q.r)
        s.qmin_size = ptr(q.min_size); s.qmax_size = ptr(q.max_size); s.qangle = ptr(q.angles); s.qoccupies = ptr(q.occupies)
        s.q_ur = ptr(q.ur); s.q_er_max = ptr(q.er_max)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        keep.append(occ)
        s.occupied = ptr(occ)
        s.th_high = float(th); s.nnratio = float(nnratio); s.check_orientation = int(bool(check_orientation)); s.mode = int(mode)
        return s, keep

    def SearchByProjection(self, matcher, queries, last_frame=False, occupied=None, qref=None):
        """matching core of FeatureMatcher::SearchByProjection(F, vpMapPoints, th) (FeatureMatcher.cc:73-154) / (CurrentFrame, LastFrame)
        (:1291-1402) against the resident frame; matcher supplies TH_HIGH / mfNNratio / mbCheckOrientation"""
        s, keep = self._queries(queries, matcher.TH_HIGH, matcher.mfNNratio, _lib.PROJ_LASTFRAME if last_frame else _lib.PROJ_LOCALMAP,
                                matcher.mbCheckOrientation, occupied, qref)
        n = self.N
        out = np.full(max(n, 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        self.ctx.check(self.lib.afv_frame_match_projection(self.handle, C.byref(s), ptr(out), ptr(nm)), "afv_frame_match_projection")
        return out[:n].copy(), int(nm[0])

    def Fuse(self, matcher, queries, use_inf_gate=True):
        s, keep = self._queries(queries, matcher.TH_LOW, matcher.mfNNratio, 0, False)
        out = np.full(max(queries.n, 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        self.ctx.check(self.lib.afv_frame_match_fuse(self.handle, C.byref(s), int(bool(use_inf_gate)), ptr(out), ptr(nm)), "afv_frame_match_fuse")
        return out[:queries.n].copy(), int(nm[0])

    def SearchForInitialization(self, matcher, F2, vbPrevMatched, windowSize=100.0):
        """SearchForInitialization(F1 = self, F2, vbPrevMatched, vnMatches12, windowSize) (FeatureMatcher.cc:399-557) between two resident
        frames; vbPrevMatched [N1, 2] float32 (not refreshed here: the caller owns it, :551-553)"""
        pm = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2)
        px, py = np.ascontiguousarray(pm[:, 0]), np.ascontiguousarray(pm[:, 1])
        n1 = self.N
        out = np.full(max(n1, 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        self.ctx.check(self.lib.afv_frame_match_initialization(self.handle, F2.handle, ptr(px), ptr(py), float(windowSize), float(matcher.TH_LOW),
                                                               float(matcher.mfNNratio), int(matcher.mbCheckOrientation), ptr(out), ptr(nm)),
                       "afv_frame_match_initialization")
        return out[:n1].copy(), int(nm[0])

    # ---- resident map points: the geometry in front of the projection searches on the device ----
    RADIUS_SCALE = 1.15  # FeatureMatcher's static radiusScale

    def set_pose(self, Rcw, tcw, Ow, fx, fy, cx, cy, mbf=0.0):
        """Frame::SetPose + the intrinsics: Rcw [3, 3], tcw [3], Ow = twc as the host computes it (Frame.cc:270-273)"""
        R = np.ascontiguousarray(Rcw, np.float32).reshape(9)
        t = np.ascontiguousarray(tcw, np.float32).reshape(3)
        o = np.ascontiguousarray(Ow, np.float32).reshape(3)
        self.ctx.check(self.lib.afv_frame_set_pose(self.handle, ptr(R), ptr(t), ptr(o), float(fx), float(fy), float(cx), float(cy), float(mbf)),
                       "afv_frame_set_pose")
        self._intrinsics = (fx, fy, cx, cy, mbf)  # what PoseOptimization hands back to set_pose with the optimised pose

    def _point_search(self, points, ids, flavour, radiusTh, viewingCosLimit=0.5, th=0.0, nnratio=0.0, check_orientation=False, qframe=None,
                      qangle=None, occupied=None, radius_scale=None):
        s = _lib.sized(_lib.PointSearch)
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        ang = None if qangle is None else np.ascontiguousarray(qangle, np.float32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        s.flavour, s.points, s.ids, s.nq = int(flavour), points.handle, ptr(ids), len(ids)
        s.radius_th, s.radius_scale = float(radiusTh), float(self.RADIUS_SCALE if radius_scale is None else radius_scale)
        s.viewing_cos_limit = float(viewingCosLimit)
        s.qframe = None if qframe is None else qframe.handle
        s.qangle, s.occupied = ptr(ang), ptr(occ)
        s.th_high, s.nnratio, s.check_orientation = float(th), float(nnratio), int(bool(check_orientation))
        return s, (ids, ang, occ)

    def project_points(self, points, ids, flavour=_lib.PT_FRUSTUM, radiusTh=1.0, viewingCosLimit=0.5, last=None, radius_scale=None):
        """afv_frame_project_points: the projection alone.  Returns a dict: in_view (bool), n_in_view, u, v, ur (mTrackProjX / Y / XR), size
        (trackSize), sigma (trackSigma), view_cos (trackViewCos), r (the window radius), qmin, qmax (the size band), er (the stereo gate); 0 where not in view"""
        s, keep = self._point_search(points, ids, flavour, radiusTh, viewingCosLimit, qframe=last, radius_scale=radius_scale)
        n = s.nq
        out = {k: np.zeros(max(n, 1), np.float32) for k in ("u", "v", "ur", "size", "sigma", "view_cos", "r", "qmin", "qmax", "er")}
        iv = np.zeros(max(n, 1), np.uint8)
        o = _lib.sized(_lib.PointProjection)
        o.in_view = ptr(iv)
        for k, a in out.items():
            setattr(o, k, ptr(a))
        self.ctx.check(self.lib.afv_frame_project_points(self.handle, C.byref(s), C.byref(o)), "afv_frame_project_points")
        res = {k: a[:n] for k, a in out.items()}
        res["in_view"] = iv[:n] != 0
        res["n_in_view"] = int(o.n_in_view)
        return res

    def isInFrustum(self, points, ids, viewingCosLimit):
        """Frame::isInFrustum (Frame.cc:276-331) of the points `ids`: mbTrackInView per id"""
        return self.project_points(points, ids, _lib.PT_FRUSTUM, 1.0, viewingCosLimit)["in_view"]

    def _search_points(self, s, keep):
        n = self.N
        out = np.full(max(n, 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        iv = np.zeros(max(s.nq, 1), np.uint8)
        niv = C.c_int32(0)
        self.ctx.check(self.lib.afv_frame_search_points(self.handle, C.byref(s), ptr(out), ptr(nm), ptr(iv), C.byref(niv)), "afv_frame_search_points")
        return out[:n].copy(), int(nm[0]), iv[:s.nq] != 0

    def SearchLocalPoints(self, matcher, points, ids, radiusTh, viewingCosLimit=0.5, occupied=None):
        """Tracking::SearchLocalPoints (Tracking.cc:988-1028): isInFrustum of every point and SearchByProjection(F, vpMapPoints, th)
        (FeatureMatcher.cc:73-154) in one call.  Returns (assign[N] = index into ids | -1, nmatches, in_view[len(ids)])"""
        s, keep = self._point_search(points, ids, _lib.PT_FRUSTUM, radiusTh, viewingCosLimit, matcher.TH_HIGH, matcher.mfNNratio, False,
                                     occupied=occupied)
        return self._search_points(s, keep)

    def SearchByProjectionLast(self, matcher, points, last, ids, radiusTh, occupied=None):
        """SearchByProjection(CurrentFrame = self, LastFrame = last, th) (FeatureMatcher.cc:1291-1402): ids[i] = the map point of the last
        frame's feature i, -1 for none / an outlier.  Returns (assign, nmatches)"""
        s, keep = self._point_search(points, ids, _lib.PT_LASTFRAME, radiusTh, 0.0, matcher.TH_HIGH, matcher.mfNNratio, matcher.mbCheckOrientation,
                                     qframe=last, occupied=occupied)
        return self._search_points(s, keep)[:2]

    def SearchByProjectionReloc(self, matcher, points, ids, radiusTh, keyframe=None, angles=None, occupied=None, useHighMatchingThreshold=False):
        """SearchByProjection(CurrentFrame = self, pKF, sAlreadyFound, th, useHigh) (FeatureMatcher.cc:1404-1506): ids[i] = the map point of
        the keyframe's feature i (-1: none / already found); the keyframe's angles from a resident frame in its role or a host array"""
        th = matcher.descDistTh_high_reloc if useHighMatchingThreshold else matcher.descDistTh_low_reloc
        s, keep = self._point_search(points, ids, _lib.PT_RELOC, radiusTh, 0.0, th, matcher.mfNNratio, matcher.mbCheckOrientation, qframe=keyframe,
                                     qangle=angles, occupied=occupied)
        return self._search_points(s, keep)[:2]

    def FusePoints(self, matcher, points, ids, radiusTh, use_inf_gate=True):
        """matching core of Fuse(pKF = self, vpMapPoints, th) (FeatureMatcher.cc:794-940; use_inf_gate False: the Sim3 flavour): returns
        (bestIdx[len(ids)] | -1, nFound)"""
        s, keep = self._point_search(points, ids, _lib.PT_FUSE, radiusTh, 0.0, matcher.TH_LOW, matcher.mfNNratio, False)
        out = np.full(max(s.nq, 1), -1, np.int32)
        nm = np.zeros(1, np.int32)
        self.ctx.check(self.lib.afv_frame_fuse_points(self.handle, C.byref(s), int(bool(use_inf_gate)), ptr(out), ptr(nm)), "afv_frame_fuse_points")
        return out[:s.nq].copy(), int(nm[0])

    # ---- Optimizer::PoseOptimization on the device ----
    def PoseOptimizationBatch(self, points, jobs):
        """afv_frame_pose_optimize over several jobs on this frame (the relocalisation loop, Tracking.cc:1247-1278: one per candidate
        keyframe).  jobs: a list of pts[N] (point id | -1; the frame's pose) or of (pts, Rcw, tcw).  Returns a list of dicts: n_good, outlier
        (bool [N]), Tcw (4 x 4 float32), Rcw, tcw, n_edges, rounds, and the per-round trace iterations, trials, chi2, lam.  The frame's
        stored pose does not change."""
        n, nj = self.N, len(jobs)
        J = (_lib.PoseJob * max(nj, 1))()
        Rs = (_lib.PoseResult * max(nj, 1))()
        keep, flags = [], np.zeros((max(nj, 1), max(n, 1)), np.uint8)
        for j, job in enumerate(jobs):
            pts, R, t = job if isinstance(job, tuple) else (job, None, None)
            pts = np.ascontiguousarray(pts, np.int32).reshape(-1)
            if len(pts) != n:
                raise ValueError("pts has %d entries, the frame %d features" % (len(pts), n))
            R = None if R is None else np.ascontiguousarray(R, np.float32).reshape(9)
            t = None if t is None else np.ascontiguousarray(t, np.float32).reshape(3)
            keep.append((pts, R, t))
            J[j].struct_size = C.sizeof(_lib.PoseJob)
            J[j].pts, J[j].Rcw, J[j].tcw = ptr(pts), ptr(R), ptr(t)
            Rs[j].struct_size = C.sizeof(_lib.PoseResult)
            Rs[j].outlier = flags[j].ctypes.data_as(C.c_void_p)
        self.ctx.check(self.lib.afv_frame_pose_optimize(self.handle, points.handle, J, nj, Rs), "afv_frame_pose_optimize")
        out = []
        for j in range(nj):
            r = Rs[j]
            Rcw, tcw = np.array(r.Rcw, np.float32).reshape(3, 3), np.array(r.tcw, np.float32)
            Tcw = np.eye(4, dtype=np.float32)
            Tcw[:3, :3], Tcw[:3, 3] = Rcw, tcw
            out.append(dict(n_good=int(r.n_good), outlier=flags[j, :n] != 0, Tcw=Tcw, Rcw=Rcw, tcw=tcw, n_edges=int(r.n_edges), rounds=int(r.rounds),
                            iterations=np.array(r.iterations, np.int32), trials=np.array(r.trials, np.int32), chi2=np.array(r.chi2, np.float64),
                            lam=np.array(r.lambda_, np.float64)))
        return out

    def PnPsolverBatch(self, points, pts_rows, **kw):
        """PnPsolver.batch on this frame (the relocalisation loop, Tracking.cc:1190-1216: one solver per candidate keyframe, one device
        call for all of them); a successful iterate gives the initial pose and the pts of a PoseOptimizationBatch job"""
        from .pnp import PnPsolver
        return PnPsolver.batch(self, points, pts_rows, **kw)

    def PoseOptimization(self, points, pts, set_pose=True):
        """Optimizer::PoseOptimization(&frame) (Optimizer.cc:245-448): pts[i] = the id of the map point of feature i | -1.  Returns
        (nGood, mvbOutlier [N] bool, Tcw 4 x 4).  set_pose: pFrame->SetPose(Tcw) (:445) - the optimised pose goes to set_pose with
        Ow = -Rcw^T tcw in float32 (Frame.cc:270-273), so the next search runs on it without the pose leaving this call."""
        r = self.PoseOptimizationBatch(points, [pts])[0]
        if set_pose:
            Rcw, tcw = r["Rcw"], r["tcw"]
            Ow = np.array([-Rcw[0, k] * tcw[0] + (-Rcw[1, k] * tcw[1] + -Rcw[2, k] * tcw[2]) for k in range(3)], np.float32)  # float32 products and sums
            self.set_pose(Rcw, tcw, Ow, *self._intrinsics)
        return r["n_good"], r["outlier"], r["Tcw"]

"""Plain-Python restatement of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth.  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of afv_table_refresh_points (include/afv_hip.h, "Refresh of resident map points"; k_refresh.hip):
the device and the host program (tools/refresh_host.cpp) are held to it bit for bit.  It follows tests/_tri_ref.py: np.float32 scalars,
one operation per statement, no fused multiply-add; the distance |XYZ - centre| and the three-term sum are that file's text (_dist, sum3).

Restated from the reference's source:

  ComputeDistinctiveDescriptors   MapPoint.cc:279-349   distinctive
      mbBad: return (:285).  No observations: return (:290).  The rows of the observations whose keyframe is not bad, in the order of the
      map<KeyframeId, Obs> (:297-306) - N rows; none: return (:308).  Distances[i][i] = 0, Distances[i][j] = DescriptorDistance (:314-324).
      Per row: sort, median = vDists[0.5 * (N - 1)] (:331-333), i.e. entry floor(0.5 (N - 1)); median < BestMedian, strict: the first row
      keeps a tie (:335).  mDescriptor = descriptors[BestIdx].clone(), refIndex, refKeyframe (:344-346).
      DescriptorDistance: the Hamming distance over the desc_bytes bytes of a binary row (pad bytes are not part of a row), or
      cv::norm(a, b, NORM_L2SQR) narrowed to float for float rows (l2sqr below: float differences, double squares, four at a time).
  UpdateNormalAndDepth            MapPoint.cc:372-418   normal_and_depth
      No observations: return (:375).  mbBad: return (:383).  EVERY observation contributes - the loop does not test isBad (:392-399):
      normal = normal + normal_i / normal_i.norm(), from vec3f::Zero(), in map order; dist = |XYZ - mpRefKF->GetCameraCenter()| (:401-402);
      refDistance = dist, refSize = GetKeyPtSize(idx of mpRefKF's observation), refSigma = GetKeyPt1DSigma = sqrt(sigma2),
      maxDistance = dist * refSize, minDistance = maxDistance / maxKeyPtSize, normalVector = normal / n (:409-416).
      It reads mpRefKF, not the refKeyframe ComputeDistinctiveDescriptors chose: the reference keeps both, and they may differ.

A point that is unset in the store is treated like a bad one (the store's rule for every routine that reads it).

Deliberate deviations:
  R1  a point whose ref keyframe is -1, or is not among its observations, gets status NO_REF and its normal part is not written (the
      reference would dereference a null Obs, :403)
  R2  a point with an observation at distance 0 or at a distance that is not finite gets status BAD_DISTANCE and its normal part is not
      written (R1 is tested first)
  R3  what is not written reads 0 in the outputs (best_obs: -1)
"""
import numpy as np

from _tri_ref import _dist, sum3  # noqa: F401  (the shared text: |X - O| = sqrt(a0 + (a1 + a2)))

f32 = np.float32
f64 = np.float64
DONE, SKIPPED, NO_OBSERVATIONS, NO_REF, BAD_DISTANCE = range(5)
STATUS_NAMES = ("done", "skipped", "no_observations", "no_ref", "bad_distance")
SET, BAD, OBSERVED = 1, 2, 4
PLANES = ("normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma")


def hamming(a, b, desc_bytes):
    return int(np.unpackbits(np.bitwise_xor(a[:desc_bytes], b[:desc_bytes])).sum())


def l2sqr(a, b):
    """normL2Sqr<float, double>: float differences, double squares, 4-way partial sums; narrowed to float"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n = len(a)
    v = (a - b).astype(np.float64)          # float differences, promoted
    q = v * v                               # double squares
    n4 = n - n % 4
    g = q[:n4].reshape(-1, 4)
    parts = ((g[:, 0] + g[:, 1]) + g[:, 2]) + g[:, 3]
    s = 0.0                                 # a Python float is a double: one rounding per +
    for t in parts.tolist() + q[n4:].tolist():
        s = s + t
    return f32(s)


# the float distance distinctive() evaluates: tests/_l2_scenes.arithmetic() puts a wrong arithmetic here (and in _proj_ref.DISTANCE) to
# prove that a scene's outcome depends on the right one
DISTANCE = {"l2sqr": l2sqr}


def median_of_row(row):
    """vDists sorted, entry floor(0.5 * (N - 1)) - by counting, not sorting: the smallest v of the row with #{d <= v} > m"""
    row = np.asarray(row)
    m = (len(row) - 1) // 2
    best = None
    for v in row:
        if np.count_nonzero(row <= v) > m and (best is None or v < best):
            best = v
    return best


def distinctive(rows, float_rows, desc_bytes):
    """rows: the N good rows in list order -> (BestIdx, BestMedian) | (-1, 0)"""
    N = len(rows)
    if N == 0:
        return -1, (f32(0.0) if float_rows else 0)
    D = [[(f32(0.0) if float_rows else 0)] * N for _ in range(N)]
    for i in range(N):
        for j in range(i + 1, N):
            d = DISTANCE["l2sqr"](rows[i], rows[j]) if float_rows else hamming(rows[i], rows[j], desc_bytes)
            D[i][j] = d
            D[j][i] = d
    best_idx, best_median = 0, None
    for i in range(N):
        med = median_of_row(D[i])
        if best_median is None or med < best_median:
            best_median, best_idx = med, i
    return best_idx, best_median


def normal_and_depth(xyz, obs, centres, ref, size_of, sigma2_of, max_size):
    """obs: [(k, idx), ...] in list order; ref: the position of mpRefKF | -1.  -> (status, fields | None)"""
    with np.errstate(all="ignore"):
        X = [f32(v) for v in xyz]
        normal = [f32(0.0)] * 3
        bad = False
        ref_idx = None
        for k, idx in obs:
            O = centres[k]
            n_i = [X[q] - f32(O[q]) for q in range(3)]
            d = _dist(X, O)
            if not np.isfinite(d) or d == 0:
                bad = True
            normal = [normal[q] + n_i[q] / d for q in range(3)]
            if k == ref:
                ref_idx = idx
        if ref < 0 or ref_idx is None:
            return NO_REF, None          # R1
        if bad:
            return BAD_DISTANCE, None    # R2
        dist = _dist(X, centres[ref])
        size = f32(size_of(ref, ref_idx))
        max_d = dist * size
        n = f32(len(obs))
        return DONE, {"normal": np.array([normal[q] / n for q in range(3)], np.float32), "ref_distance": dist, "ref_size": size,
                      "ref_sigma": np.sqrt(f32(sigma2_of(ref, ref_idx))), "max_distance": max_d, "min_distance": max_d / f32(max_size[ref])}


def refresh(scene, descriptors=True, normals=True):
    """scene: see _refresh_scenes.Scene.  -> (status [np] int32, best_obs [np] int32 (an index into scene.observations | -1), best_median
    [np], store: {id: fields after the call} for EVERY id of the scene's store)"""
    store = {i: {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in f.items()} for i, f in scene.store.items()}
    npts = len(scene.point_ids)
    status, best_obs = np.zeros(npts, np.int32), np.full(npts, -1, np.int32)
    best_median = np.zeros(npts, np.float32 if scene.float_dim else np.int32)
    where_k = {s: i for i, s in enumerate(scene.kfs)}
    bad_kf = set(scene.kf_bad)
    for p, pid in enumerate(scene.point_ids):
        fields = store[pid]
        mine = [(e, where_k[s], idx) for e, (q, s, idx) in enumerate(scene.observations) if q == pid]
        if not (fields["flags"] & SET) or (fields["flags"] & BAD):
            status[p] = SKIPPED
            continue
        if not mine:
            status[p] = NO_OBSERVATIONS
            continue
        if descriptors:
            good = [(e, k, idx) for e, k, idx in mine if scene.kfs[k] not in bad_kf]
            rows = [scene.rows[scene.kfs[k]][idx] for _, k, idx in good]
            bi, bm = distinctive(rows, bool(scene.float_dim), scene.desc_bytes)
            if bi >= 0:
                best_obs[p], best_median[p] = good[bi][0], bm
                fields["descriptors"] = np.array(rows[bi][:scene.desc_bytes] if not scene.float_dim else rows[bi], copy=True)
        if normals:
            centres = [scene.centres[s] for s in scene.kfs]
            max_size = [scene.max_size[s] for s in scene.kfs]
            ref = where_k.get(scene.ref_kf.get(pid, -1), -1)
            st, out = normal_and_depth(fields["pos"], [(k, idx) for _, k, idx in mine], centres, ref,
                                       lambda k, idx: scene.size[scene.kfs[k]][idx], lambda k, idx: scene.sigma2[scene.kfs[k]][idx], max_size)
            status[p] = st
            if out is not None:
                fields.update(out)
    return status, best_obs, best_median, store

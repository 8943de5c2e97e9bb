"""-m gpu: keyframe tables of float descriptors (afv_table_create_f32): SIFT128 / SURF64 / KAZE64-like rows at the templated dimensions
(64, 128, 256) and at two run-time ones (36, 200).  Bar: every match vector / count equal to the CPU oracle, bit for bit - the oracle
evaluates L2^2 in cv::norm's summation order at any dimension and applies the rotation histogram.  Both row kinds of _float_desc: 0/1
values (equal distances everywhere) and full mantissas (the summation order shows)."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _float_desc import floaten  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [64, 128, 256, 36, 200]
AFV_EINVAL = -1         # include/afv_hip.h
AFV_EUNSUPPORTED = -6
PAIR_CAP = 600
PAIR_SIZES = [600, 600, 1, 63, 64, 65, 0]                       # slots 0 .. 6: two full sets, the ragged ones, an empty one
PAIRS = [(0, 1), (1, 0), (0, 0), (2, 0), (0, 2), (3, 4), (4, 5), (5, 3), (6, 0), (0, 6), (1, 1), (3, 3), (5, 1), (1, 4)]


@pytest.fixture(scope="module")
def tbl(afv):
    return importlib.import_module("anyfeature-vslam_amd.table")


@pytest.fixture(scope="module")
def ctx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context()
    yield c
    c.close()


# ---------------- data (used by tests/test_table_float_cpu.py as well, which proves on the oracle that they reach their branches) ------
def _clustered(afv, seed, n, nproto=20, maxflips=24):
    """n 32-byte rows near `nproto` prototypes (0 .. `maxflips` flipped bits each): many near-equal neighbours per row, so a row's 4
    nearest columns are often taken by earlier rows and the greedy rule has to look further (with 6 flips on every row the 0/1 variant at
    128 floats never got there: tests/test_table_float_cpu.py counts such rows)"""
    s = afv.synth
    proto = np.unpackbits(s.random_descriptors(4000, nproto, 32), axis=1)      # the same prototypes for every seed
    which = s.lcg_states(seed, n) % nproto
    nflip = s.lcg_states(seed + 2, n) % (maxflips + 1)
    pos = (s.lcg_states(seed + 1, n * maxflips) % 256).reshape(n, maxflips)
    bits = proto[which].copy()
    for f in range(maxflips):
        sel = np.nonzero(nflip > f)[0]
        bits[sel, pos[sel, f]] ^= 1
    return np.packbits(bits, axis=1)


def pair_data(afv, dim, real):
    """rows[slot] (float32, (n, dim)), angles[slot], th_low (the 0.2 quantile of the distances between slots 0 and 1)"""
    s = afv.synth
    rows, angles = [], []
    for k, n in enumerate(PAIR_SIZES):
        rows.append(floaten(_clustered(afv, 100 + 10 * k, max(n, 1)), dim, real)[:n])
        angles.append((s.lcg_states(900 + k, max(n, 1))[:n] % 360).astype(np.float32))
    a, b = rows[0].astype(np.float64), rows[1].astype(np.float64)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)     # (a threshold, not a distance the matchers see)
    return rows, angles, float(np.float32(np.quantile(d, 0.2)))


def _th(dim, real):
    return 75.0 * dim / 256.0 * (0.6 if real else 1.0)


def guided_data(afv, dim, real, K=8, cap=300):
    """the config #4 recipe (keyframe k + 1 = keyframe k with bits flipped and rows replaced) as float rows, ragged counts, an empty slot and
    a slot of one feature; FeatureVectors over 25 nodes, geometry, validity masks on every third slot"""
    s = afv.synth
    t32, ang, cnt = s.keyframe_table(K, cap, seed=3, nbytes=32)
    cnt = cnt.copy()
    for k in range(K):
        cnt[k] = max(cap - (k * 37) % max(cap // 3, 1), 0)
    cnt[1], cnt[2] = 0, 1
    t = np.stack([floaten(t32[k], dim, real) for k in range(K)])
    x0 = (s.lcg_states(300, cap) % 60000).astype(np.float32) / 100.0
    y0 = (s.lcg_states(400, cap) % 47000).astype(np.float32) / 100.0
    sg0 = ((np.float32(1.2) ** (s.lcg_states(500, cap) % 8).astype(np.float32)) ** 2).astype(np.float32)
    fvs, geo, valid = [], [], [None] * K
    for k in range(K):
        n = int(cnt[k])
        fvs.append(_featvec(afv, 90, n, 25))
        geo.append((x0[:n] + np.float32(2 * k), y0[:n].copy(), sg0[:n].copy()))
        if k % 3 == 0:
            valid[k] = (s.lcg_bytes(700 + k, max(n, 1))[:n] > 60).astype(np.uint8)
    return t32, t, ang, cnt, fvs, geo, valid


def _featvec(afv, seed, n, nnodes):
    node_of = afv.synth.lcg_states(seed, max(n, 1))[:n] % nnodes
    fv = []
    for k in range(nnodes):
        idx = np.nonzero(node_of == k)[0]
        if len(idx):
            fv.append((int(k * 3 + 1), idx.tolist()))
    return fv


def _csr(fv):
    ids = np.array([k for k, _ in fv], np.int32)
    ptr = np.zeros(len(fv) + 1, np.int32)
    for i, (_, v) in enumerate(fv):
        ptr[i + 1] = ptr[i] + len(v)
    idx = np.array([x for _, v in fv for x in v], np.int32)
    return ids, ptr, idx


def _fill_pairs(tbl, ctx, dim, rows, angles):
    table = tbl.DescriptorTable(ctx, len(PAIR_SIZES), PAIR_CAP, float_dim=dim)
    for k, r in enumerate(rows):
        table.set(k, r.reshape(-1, dim), angles[k])
    return table


# ---------------- brute-force pairs ----------------
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_pairs(afv, oracle, tbl, ctx, dim, real):
    """match_pairs and match_pairs_device against SearchByBoW(KF,KF) without nodes: with and without the rotation histogram, nnratio 0.75
    and 1.0, ragged sets (1, 63, 64, 65, cap), an empty set, pairs (a, a); one pair alone, and the whole list cut into chunks of 4 jobs"""
    import torch
    rows, angles, th = pair_data(afv, dim, real)
    table = _fill_pairs(tbl, ctx, dim, rows, angles)
    assert table.float_dim == dim and table.pitch == 4 * dim
    pa = np.array([a for a, _ in PAIRS], np.int32)
    pb = np.array([b for _, b in PAIRS], np.int32)
    total = 0
    try:
        d = table.device_views()[0]
        assert d.dtype == torch.float32 and tuple(d.shape) == (len(PAIR_SIZES), PAIR_CAP, dim)
        assert np.array_equal(d[1, :PAIR_SIZES[1]].cpu().numpy(), rows[1])
        for ori in (False, True):
            for ratio in (0.75, 1.0):
                want = [oracle.search_by_bow_kf_kf(rows[a], rows[b], angle1=angles[a], angle2=angles[b], th_low=th, nnratio=ratio,
                                                   check_orientation=ori) for a, b in PAIRS]
                total += sum(w[1] for w in want)
                m, nm = table.match_pairs(pa[:1], pb[:1], th, ratio, ori)           # one pair alone
                assert nm[0] == want[0][1] and np.array_equal(m[0, :PAIR_SIZES[0]], want[0][0]), (dim, real, ori, ratio)
                for chunk in (2048, 4):                                             # one launch pair, then four
                    ctx.set_l2_chunk_pairs(chunk)
                    m, nm = table.match_pairs(pa, pb, th, ratio, ori)
                    dm, dn = table.match_pairs_device(torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), th, ratio, ori)
                    torch.cuda.synchronize()
                    dm, dn = dm.cpu().numpy(), dn.cpu().numpy()
                    for p, (a, b) in enumerate(PAIRS):
                        wm, wn = want[p]
                        assert nm[p] == wn and dn[p] == wn, (dim, real, ori, ratio, chunk, p)
                        assert np.array_equal(m[p, :PAIR_SIZES[a]], wm) and np.array_equal(dm[p, :PAIR_SIZES[a]], wm), (dim, real, ori, ratio, chunk, p)
                        assert np.all(m[p, PAIR_SIZES[a]:] == -1) and np.all(dm[p, PAIR_SIZES[a]:] == -1)
    finally:
        ctx.set_l2_chunk_pairs(2048)
        table.close()
    assert total > 100


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("dim", [64, 128])
def test_pairs_equal_the_raw_array_matcher(afv, tbl, ctx, dim, real):
    """without orientation the table's answer is afv_match_l2_pairs_device's on the same rows"""
    import torch
    rows, angles, th = pair_data(afv, dim, real)
    table = _fill_pairs(tbl, ctx, dim, rows, angles)
    try:
        d, _, n = table.device_views()
        pa = torch.tensor([a for a, _ in PAIRS], dtype=torch.int32, device="cuda")
        pb = torch.tensor([b for _, b in PAIRS], dtype=torch.int32, device="cuda")
        for ratio in (0.75, 1.0):
            tm, tn = table.match_pairs_device(pa, pb, th, ratio, False)
            rm, rn = afv.FeatureMatcher(ratio, False, ctx=ctx).match_l2_pairs_device(d, n, pa, pb, th)
            torch.cuda.synchronize()
            assert torch.equal(tn, rn) and torch.equal(tm, rm) and int(tn.sum()) > 50
    finally:
        table.close()


# ---------------- BoW-guided searches and triangulation ----------------
def _tri_vec(wm, na):
    if isinstance(wm, np.ndarray) and wm.ndim == 2:
        vec = np.full(na, -1, np.int32)
        for i1, i2 in wm:
            vec[i1] = i2
        return vec
    return wm


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_bow_relocalisation_and_triangulation(afv, oracle, tbl, ctx, dim, real):
    """match_bow with validity masks, match_bow_frame with a host frame view and match_triangulation (monocular, stereo, has-map-point
    masks); a slot that lacks its FeatureVector or its geometry is refused with AFV_EINVAL"""
    s = afv.synth
    K, cap = 8, 300
    t32, t, ang, cnt, fvs, geo, valid = guided_data(afv, dim, real, K, cap)
    th = _th(dim, real)
    table = tbl.DescriptorTable(ctx, K, cap, float_dim=dim)
    try:
        for k in range(K):
            table.set(k, t[k, :cnt[k]], ang[k, :cnt[k]])
        pa = np.array([k for k in range(K) for _ in range(2)], np.int32)
        pb = np.array([(k + 1 + j) % K for k in range(K) for j in range(2)], np.int32)
        with pytest.raises(afv._lib.AfvError) as e:      # no FeatureVector was ever stored
            table.match_bow(pa, pb, th, 0.75, True)
        assert e.value.code == AFV_EINVAL
        for k in range(K):
            if k != 5:
                table.set_featvec(k, *_csr(fvs[k]))
        with pytest.raises(afv._lib.AfvError) as e:      # slot 5 holds features but no FeatureVector
            table.match_bow(pa, pb, th, 0.75, True)
        assert e.value.code == AFV_EINVAL
        table.set_featvec(5, *_csr(fvs[5]))
        for k in range(K):
            if valid[k] is not None:
                table.set_valid(k, valid[k])
        # SearchByBoW(KF, KF)
        for ori in (False, True):
            m, nm = table.match_bow(pa, pb, th, 0.75, ori)
            total = 0
            for p in range(len(pa)):
                a, b = int(pa[p]), int(pb[p])
                wm, wn = oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], fvs[a], fvs[b], valid[a], valid[b], ang[a, :cnt[a]],
                                                    ang[b, :cnt[b]], th, 0.75, ori)
                assert nm[p] == wn and np.array_equal(m[p, :cnt[a]], wm), (dim, real, ori, p)
                total += wn
            assert total > 20
        # SearchByBoW(KF, F): keyframe 4 seen again
        nf = 200
        fdesc = floaten(s.perturbed_descriptors(t32[4, :nf].copy(), 4242), dim, real)
        fang = ((ang[4, :nf] + 3.0) % 360.0).astype(np.float32)
        ffv = _featvec(afv, 90, nf, 25)
        slots = np.arange(K, dtype=np.int32)[::-1].copy()
        m, nm = table.match_bow_frame(slots, afv.FeatureView(fdesc, ffv, None, fang), th, 0.75, True)
        for p, k in enumerate(slots):
            wm, wn = oracle.search_by_bow_kf_frame(t[k, :cnt[k]], fdesc, fvs[k], ffv, valid[k], ang[k, :cnt[k]], fang, th, 0.75, True)
            assert nm[p] == wn and np.array_equal(m[p], wm), (dim, real, p, k)
        assert nm[list(slots).index(4)] > 20
        # SearchForTriangulation: no geometry yet, then monocular, then with u_right on every keyframe and has-map-point masks
        F = np.tile(np.array([0, 0, 0, 0, 0, -1, 1e-4, 1, 0], np.float32), (len(pa), 1))
        ep = np.tile(np.array([1.0e6, 240.0], np.float32), (len(pa), 1))
        with pytest.raises(afv._lib.AfvError) as e:
            table.match_triangulation(pa, pb, F, ep, th)
        assert e.value.code == AFV_EINVAL
        for k in range(K):
            if k != 3:
                table.set_geometry(k, *geo[k])
        with pytest.raises(afv._lib.AfvError) as e:      # slot 3 lacks its geometry
            table.match_triangulation(pa, pb, F, ep, th)
        assert e.value.code == AFV_EINVAL
        table.set_geometry(3, *geo[3])
        mp1 = [(s.lcg_bytes(800 + p, max(int(cnt[pa[p]]), 1))[:cnt[pa[p]]] > 200).astype(np.uint8) for p in range(len(pa))]
        mp2 = [(s.lcg_bytes(850 + p, max(int(cnt[pb[p]]), 1))[:cnt[pb[p]]] > 200).astype(np.uint8) for p in range(len(pa))]
        for stereo, masks in ((False, False), (True, False), (True, True)):
            if stereo:
                for k in range(K):
                    table.set_geometry(k, *geo[k], u_right=geo[k][0] - np.float32(30.0))
            m, nm = table.match_triangulation(pa, pb, F, ep, th, mp1 if masks else None, mp2 if masks else None)
            total = 0
            for p in range(len(pa)):
                a, b = int(pa[p]), int(pb[p])
                na, nb = int(cnt[a]), int(cnt[b])
                pts1 = np.stack([geo[a][0], geo[a][1]], 1) if na else np.zeros((0, 2), np.float32)
                pts2 = np.stack([geo[b][0], geo[b][1]], 1) if nb else np.zeros((0, 2), np.float32)
                kw = {}
                if stereo:
                    kw = dict(u_right1=geo[a][0] - np.float32(30.0), u_right2=geo[b][0] - np.float32(30.0))
                wm, wn = oracle.search_for_triangulation(t[a, :na], t[b, :nb], pts1, pts2, geo[b][2], F[p].reshape(3, 3), ep[p], fvs[a], fvs[b],
                                                         mp1[p] if masks else None, mp2[p] if masks else None, th, **kw)
                assert nm[p] == wn, (dim, real, stereo, masks, p)
                assert np.array_equal(m[p, :na], _tri_vec(wm, na)), (dim, real, stereo, masks, p)
                total += wn
            assert total > 20, (stereo, masks)
    finally:
        table.close()


# ---------------- resident float frames into the table ----------------
@pytest.mark.parametrize("dim", [128, 64, 256])
def test_resident_float_frames_into_the_table(afv, oracle, tbl, ctx, dim):
    """float frame -> ComputeBoW on a float vocabulary -> set_from_frame: the slot equals a slot filled with set + set_featvec +
    set_geometry in every output (pairs, BoW, relocalisation, triangulation); match_bow_frame_resident equals the oracle; a
    SearchByProjection whose queries name table rows equals the same search with the descriptors passed by value"""
    img = afv.synth.corners_frame(9)
    k1, d1 = ctx.extract(img)
    k2, d2 = ctx.extract(np.roll(img, 4, axis=1))
    f1d, f2d = floaten(d1, dim, True), floaten(d2, dim, True)
    th = _th(dim, True)
    voc = afv.Vocabulary.random_float(5, k=8, L=3, ctx=ctx, dim=dim)
    f1, f2 = afv.Frame(ctx, float_dim=dim), afv.Frame(ctx, float_dim=dim)
    f1.set_features(k1, f1d)
    f2.set_features(k2, f2d)
    _, fv1 = f1.ComputeBoW(voc, levelsup=2)
    _, fv2 = f2.ComputeBoW(voc, levelsup=2)
    cap = max(len(k1), len(k2))
    table = tbl.DescriptorTable(ctx, 4, cap, float_dim=dim)
    afv.FeatureMatcher.setDescriptorDistanceThresholds(th)
    try:
        table.set_from_frame(0, f1)
        table.set_from_frame(1, f2)
        d, _, n = table.device_views()
        d = d.cpu().numpy()
        assert np.array_equal(d[0, :len(f1d)], f1d) and np.array_equal(d[1, :len(f2d)], f2d)
        assert list(n.cpu().numpy()[:2]) == [len(k1), len(k2)]
        # the same two keyframes from host arrays: slots 2 and 3
        _, sig1, _ = ctx.size_sigma(k1)
        _, sig2, _ = ctx.size_sigma(k2)
        for slot, k, fd, fv, sg in ((2, k1, f1d, fv1, sig1), (3, k2, f2d, fv2, sig2)):
            table.set(slot, fd, k["angle"])
            table.set_featvec(slot, *_csr(fv))
            table.set_geometry(slot, k["x"], k["y"], sg)
        A, B = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
        F = np.tile(np.array([0, 0, 0, 0, 0, -1, 1e-4, 1, 0], np.float32), (2, 1))
        ep = np.tile(np.array([1.0e6, 240.0], np.float32), (2, 1))
        for name, call in (("pairs", lambda a, b: table.match_pairs(a, b, th, 0.75, True)),
                           ("bow", lambda a, b: table.match_bow(a, b, th, 0.75, True)),
                           ("tri", lambda a, b: table.match_triangulation(a, b, F, ep, th))):
            r0, r1 = call(A, B), call(A + 2, B + 2)
            assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1]) and r0[1].sum() > 50, (dim, name)
        r0 = table.match_bow_frame_resident(np.array([0, 2], np.int32), f2, th, 0.75, True)
        assert np.array_equal(r0[0][0], r0[0][1]) and r0[1][0] == r0[1][1]
        # ... and against the oracle
        m, nm = table.match_pairs(A[:1], B[:1], th, 0.75, True)
        wm, wn = oracle.search_by_bow_kf_kf(f1d, f2d, angle1=k1["angle"], angle2=k2["angle"], th_low=th, nnratio=0.75, check_orientation=True)
        assert nm[0] == wn and np.array_equal(m[0, :len(f1d)], wm) and wn > 100
        m, nm = table.match_bow(A[:1], B[:1], th, 0.75, True)
        wm, wn = oracle.search_by_bow_kf_kf(f1d, f2d, fv1, fv2, None, None, k1["angle"], k2["angle"], th, 0.75, True)
        assert nm[0] == wn and np.array_equal(m[0, :len(f1d)], wm)
        wm, wn = oracle.search_by_bow_kf_frame(f1d, f2d, fv1, fv2, None, k1["angle"], k2["angle"], th, 0.75, True)
        assert r0[1][0] == wn and np.array_equal(r0[0][0], wm)
        # projection queries naming rows of slot 0, against frame 2, equal the same queries by value
        size1, _, _ = ctx.size_sigma(k1)
        pick = np.argsort(afv.synth.lcg_states(3, len(k1)), kind="stable")[:500]
        u = k1["x"][pick] + np.float32(4); v = k1["y"][pick]
        Q = afv.ProjectionQueries(f1d[pick], u, v, np.float32(15) * size1[pick], size1[pick] / np.float32(1.2), size1[pick] * np.float32(1.2),
                                  angles=k1["angle"][pick])
        mt = afv.FeatureMatcher(0.9, True, ctx=ctx)
        byval, nv = f2.SearchByProjection(mt, Q, last_frame=True)
        byref, nr = f2.SearchByProjection(mt, Q, last_frame=True, qref=(table, np.zeros(len(pick), np.int32), pick.astype(np.int32)))
        assert nv == nr and np.array_equal(byval, byref) and nv > 100
    finally:
        table.close(); f1.close(); f2.close(); voc.close()
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)


# ---------------- replication ----------------
def _replica_source(afv, tbl, ctx, dim):
    K, cap = 8, 300
    t32, t, ang, cnt, fvs, geo, valid = guided_data(afv, dim, True, K, cap)
    src = tbl.DescriptorTable(ctx, K, cap, float_dim=dim)
    for k in range(K):
        src.set(k, t[k, :cnt[k]], ang[k, :cnt[k]])
        src.set_featvec(k, *_csr(fvs[k]))
        src.set_geometry(k, *geo[k], u_right=geo[k][0] - np.float32(30.0))
        if valid[k] is not None:
            src.set_valid(k, valid[k])
    return src, (t, ang, cnt, fvs)


def _replica_outputs(table, dim):
    K = 8
    pa = np.array([k for k in range(K) for _ in range(2)], np.int32)
    pb = np.array([(k + 1 + j) % K for k in range(K) for j in range(2)], np.int32)
    F = np.tile(np.array([0, 0, 0, 0, 0, -1, 1e-4, 1, 0], np.float32), (len(pa), 1))
    ep = np.tile(np.array([1.0e6, 240.0], np.float32), (len(pa), 1))
    th = _th(dim, True)
    return [table.match_pairs(pa, pb, th, 0.75, True), table.match_bow(pa, pb, th, 0.75, True), table.match_triangulation(pa, pb, F, ep, th)]


def test_clone(afv, oracle, tbl, ctx):
    """clone_into a second context reproduces every output; a clone between a 64-byte binary table and a table of 16 floats (same pitch,
    same byte size) or between two float dimensions is refused with AFV_EUNSUPPORTED"""
    dim = 128
    src, (t, ang, cnt, fvs) = _replica_source(afv, tbl, ctx, dim)
    ctx2 = afv.Context()
    dst = tbl.DescriptorTable(ctx2, 8, 300, float_dim=dim)
    b64 = tbl.DescriptorTable(ctx2, 8, 300, desc_bytes=64)
    f16 = tbl.DescriptorTable(ctx2, 8, 300, float_dim=16)
    f64 = tbl.DescriptorTable(ctx2, 8, 300, float_dim=64)
    comm = tbl.Communicator(ctx, 0, 1, lambda ident: ident)
    try:
        assert b64.pitch == f16.pitch == 64
        b64.set(0, np.full((5, 64), 0xAB, np.uint8))
        f16.set(0, np.full((7, 16), 2.5, np.float32))
        for a, b in ((b64, f16), (f16, b64), (src, f64), (f64, src), (src, b64)):
            with pytest.raises(afv._lib.AfvError) as e:
                a.clone_into(b)
            assert e.value.code == AFV_EUNSUPPORTED
        for tab, rows, val in ((b64, 5, 0xAB), (f16, 7, 2.5)):   # nothing moved
            d, _, n = tab.device_views()
            assert np.all(d[0, :rows].cpu().numpy() == val) and list(n.cpu().numpy()) == [rows] + [0] * 7
        src.clone_into(dst)
        assert src.broadcast(comm, root=0) >= 0.0           # a world of one
        for r0, r1 in zip(_replica_outputs(src, dim), _replica_outputs(dst, dim)):
            assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1]) and r0[1].sum() > 20
        wm, wn = oracle.search_by_bow_kf_kf(t[0, :cnt[0]], t[3, :cnt[3]], fvs[0], fvs[3], None, None, ang[0, :cnt[0]], ang[3, :cnt[3]],
                                            _th(dim, True), 0.75, True)
        dst.set_valid(0, None); dst.set_valid(3, None)
        m, nm = dst.match_bow(np.array([0], np.int32), np.array([3], np.int32), _th(dim, True), 0.75, True)
        assert nm[0] == wn and np.array_equal(m[0, :cnt[0]], wm)
    finally:
        comm.close(); src.close(); dst.close(); b64.close(); f16.close(); f64.close(); ctx2.close()


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)   # host channel for the id only
    afv = importlib.import_module("anyfeature-vslam_amd")
    tbl = importlib.import_module("anyfeature-vslam_amd.table")

    def exchange(ident):
        box = [ident]
        dist.broadcast_object_list(box, src=0)
        return box[0]
    ctx = afv.Context(device=rank)
    comm = tbl.Communicator(ctx, rank, world, exchange)
    # rank 0 holds 64-byte binary rows, rank 1 rows of 16 floats: same pitch, same byte size - refused on EVERY rank before data moves
    odd = tbl.DescriptorTable(ctx, 8, 300, desc_bytes=64) if rank == 0 else tbl.DescriptorTable(ctx, 8, 300, float_dim=16)
    if rank == 0:
        odd.set(0, np.full((5, 64), 0xAB, np.uint8))
    else:
        odd.set(0, np.full((7, 16), 2.5, np.float32))
    code = 0
    try:
        odd.broadcast(comm, root=0)
    except afv._lib.AfvError as e:
        code = e.code
    d, _, n = odd.device_views()
    rows, val = (5, 0xAB) if rank == 0 else (7, 2.5)
    untouched = bool(np.all(d[0, :rows].cpu().numpy() == val)) and list(n.cpu().numpy()) == [rows] + [0] * 7
    q.put(("refused", rank, code, untouched))
    odd.close()
    dim = 128
    if rank == 0:
        table, _ = _replica_source(afv, tbl, ctx, dim)
    else:
        table = tbl.DescriptorTable(ctx, 8, 300, float_dim=dim)
    table.broadcast(comm, root=0)
    out = _replica_outputs(table, dim)
    q.put(("outputs", rank, [(m.tobytes(), nm.tolist()) for m, nm in out]))
    table.close()
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_broadcast_two_ranks(afv):
    """a float table broadcast in a world of 2: the replica answers like the root; 64-byte binary rows against 16 floats are refused on
    both ranks with AFV_EUNSUPPORTED and nothing moves.  Needs two GPUs (skipped on a host with one)."""
    import torch
    import torch.multiprocessing as mp
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    msgs = [q.get(timeout=500) for _ in range(4)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    refused = sorted(m for m in msgs if m[0] == "refused")
    assert [m[2] for m in refused] == [AFV_EUNSUPPORTED, AFV_EUNSUPPORTED] and all(m[3] for m in refused)
    outs = sorted((m for m in msgs if m[0] == "outputs"), key=lambda m: m[1])
    assert outs[0][2] == outs[1][2] and sum(outs[0][2][1][1]) > 20


# ---------------- refusals ----------------
def test_refusals(afv, tbl, ctx):
    """kind and dimension mismatches between frames and tables: AFV_EUNSUPPORTED, and the table keeps what it held"""
    img = afv.synth.corners_frame(9)
    k1, d1 = ctx.extract(img)
    n = len(k1)
    fb = afv.Frame(ctx)                                   # a binary frame (32 bytes) after ComputeBoW
    fb.set_features(k1, d1)
    bvoc = afv.Vocabulary.random(5, k=8, L=3, ctx=ctx)
    fb.ComputeBoW(bvoc, levelsup=2)
    ff = {}
    vocs = []
    for dim in (64, 128):
        ff[dim] = afv.Frame(ctx, float_dim=dim)
        ff[dim].set_features(k1, floaten(d1, dim, True))
        vocs.append(afv.Vocabulary.random_float(5, k=8, L=3, ctx=ctx, dim=dim))
        ff[dim].ComputeBoW(vocs[-1], levelsup=2)
    f8 = afv.Frame(ctx, float_dim=8)                      # 8 floats = 32 bytes: the byte size of an ORB32 row
    f8.set_features(k1, floaten(d1, 8, True))
    t32 = tbl.DescriptorTable(ctx, 2, n)
    t128 = tbl.DescriptorTable(ctx, 2, n, float_dim=128)
    t8 = tbl.DescriptorTable(ctx, 2, n, float_dim=8)
    mark = np.full((3, 128), 7.0, np.float32)
    try:
        t128.set(0, mark)
        t32.set(0, d1[:3])
        cases = [(t128, fb), (t128, ff[64]), (t32, ff[128]), (t32, f8), (t8, fb)]
        for t, f in cases:
            with pytest.raises(afv._lib.AfvError) as e:
                t.set_from_frame(0, f)
            assert e.value.code == AFV_EUNSUPPORTED
        for t, f in ((t128, fb), (t128, ff[64]), (t32, ff[128])):
            with pytest.raises(afv._lib.AfvError) as e:
                t.match_bow_frame_resident(np.array([0], np.int32), f, 10.0, 0.75)
            assert e.value.code == AFV_EUNSUPPORTED
        d, _, cnt = t128.device_views()
        assert np.array_equal(d[0, :3].cpu().numpy(), mark) and list(cnt.cpu().numpy()) == [3, 0]
        assert np.array_equal(t32.device_views()[0][0, :3].cpu().numpy(), d1[:3])
        # queries naming rows of a table of another kind / dimension
        size1, _, _ = ctx.size_sigma(k1)
        ref = (np.zeros(3, np.int32), np.arange(3, dtype=np.int32))
        mt = afv.FeatureMatcher(0.9, True, ctx=ctx)
        for f, t, rows in ((ff[64], t128, floaten(d1, 64, True)), (ff[128], t32, floaten(d1, 128, True)), (fb, t128, d1), (f8, t32, floaten(d1, 8, True))):
            Q = afv.ProjectionQueries(rows[:3], k1["x"][:3], k1["y"][:3], np.float32(15) * size1[:3], size1[:3], size1[:3])
            with pytest.raises(afv._lib.AfvError) as e:
                f.SearchByProjection(mt, Q, last_frame=True, qref=(t,) + ref)
            assert e.value.code == AFV_EUNSUPPORTED
    finally:
        for x in [t32, t128, t8, fb, f8, bvoc] + list(ff.values()) + vocs:
            x.close()


def test_wrong_rows_raise_before_the_library(afv, tbl, ctx):
    t = tbl.DescriptorTable(ctx, 2, 16, float_dim=64)
    try:
        for bad in (np.zeros((4, 128), np.float32), np.zeros((4, 64), np.uint8), np.zeros((4, 256), np.uint8), np.zeros(64 * 4, np.float32),
                    np.zeros((4, 64), np.float64)):
            with pytest.raises(ValueError):
                t.set(0, bad)
        for bad in (np.zeros((4, 128), np.float32), np.zeros((4, 64), np.uint8)):
            with pytest.raises(ValueError):
                t.match_bow_frame(np.array([0], np.int32), afv.FeatureView(bad), 1.0, 0.75)
        with pytest.raises(ValueError):
            t.upload(np.zeros((2, 16, 64), np.uint8), np.zeros((2, 16), np.float32), np.zeros(2, np.int32))
        host = (np.arange(2 * 16 * 64, dtype=np.float32).reshape(2, 16, 64), np.zeros((2, 16), np.float32), np.array([16, 5], np.int32))
        t.upload(*host)
        d, _, n = t.device_views()
        assert np.array_equal(d.cpu().numpy(), host[0]) and list(n.cpu().numpy()) == [16, 5]
    finally:
        t.close()

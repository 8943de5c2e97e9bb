"""-m gpu: BASELINE.json configs[3] — keyframe descriptor table resident in HBM, pair-job batches, the C-ABI RCCL
communicator.  Bar: every match vector / count equal to the CPU oracle's SearchByBoW / SearchForTriangulation."""
import importlib
import os
import socket
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, RATIO = 75.0, 0.75


@pytest.fixture(scope="module")
def tbl(afv):
    return importlib.import_module("anyfeature-vslam_amd.table")


@pytest.fixture(scope="module")
def dist_mod(afv):
    return importlib.import_module("anyfeature-vslam_amd.dist")


def _oracle_job(oracle, host, a, b, ori=True, ratio=RATIO):
    t, ang, cnt = host
    return oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], angle1=ang[a, :cnt[a]], angle2=ang[b, :cnt[b]], th_low=TH, nnratio=ratio,
                                      check_orientation=ori)


@pytest.mark.timeout(900)
def test_config4_full_size_10k_jobs(afv, oracle, tbl, dist_mod):
    """K = 1000 keyframes x 1000 x 32 B, 10 000 LCG pair jobs on one GPU: EVERY job count and 128 full match
    vectors against the oracle; plus the covisible job list, whose jobs really match."""
    import torch
    K, cap, njobs = 1000, 1000, 10000
    host = afv.synth.keyframe_table(K, cap)
    ctx = afv.Context()
    table = tbl.DescriptorTable(ctx, K, cap)
    table.upload(*host)
    a, b = dist_mod.lcg_pairs(12345, njobs, K)
    bc = ((a.astype(np.int64) + 1 + (b.astype(np.int64) % 3)) % K).astype(np.int32)
    for kind, pb in (("uniform", b), ("covisible", bc)):
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(pb).cuda()
        match, nm = table.match_pairs_device(d_a, d_b, TH, RATIO, True)
        torch.cuda.synchronize()
        nm = nm.cpu().numpy()
        check = range(njobs) if kind == "uniform" else range(0, njobs, 20)   # the covisible oracle jobs walk ~500 matches each
        with ThreadPoolExecutor(max(os.cpu_count() or 4, 4)) as ex:          # ctypes releases the GIL inside the oracle
            want = list(ex.map(lambda j: _oracle_job(oracle, host, int(a[j]), int(pb[j])), check))
        for j, (wm, wn) in zip(check, want):
            assert nm[j] == wn, (kind, j, int(a[j]), int(pb[j]))
        full = list(check)[::max(len(list(check)) // 128, 1)][:128]
        got = match[torch.tensor(full, device="cuda")].cpu().numpy()
        lut = dict(zip(check, want))
        for r, j in enumerate(full):
            assert np.array_equal(got[r], lut[j][0]), (kind, j)
        if kind == "covisible":
            assert nm.mean() > 100            # overlapping keyframes: hundreds of matches per job
    # the host-array entry point returns the same thing
    m2, nm2 = table.match_pairs(a[:64], bc[:64], TH, RATIO, True)
    ref = table.match_pairs_device(torch.from_numpy(a[:64]).cuda(), torch.from_numpy(bc[:64]).cuda(), TH, RATIO, True)
    torch.cuda.synchronize()
    assert np.array_equal(m2, ref[0].cpu().numpy()) and np.array_equal(nm2, ref[1].cpu().numpy())
    table.close()
    ctx.close()


def _small_table(afv, K=24, cap=384):
    t, ang, cnt = afv.synth.keyframe_table(K, cap, seed=3)
    cnt = cnt.copy()
    for k in range(K):                       # ragged: different feature counts, one empty keyframe
        cnt[k] = cap - (k * 13) % 90
    cnt[5] = 0
    return t, ang, cnt


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


@pytest.mark.parametrize("ori", [False, True])
def test_table_bow_guided_pairs(afv, oracle, tbl, ori):
    """device-resident BoW-guided SearchByBoW(KF,KF) (FeatureMatcher.cc:561-660): merge-join on the host, descriptors and
    feature indices in HBM"""
    host = _small_table(afv)
    t, ang, cnt = host
    K = len(cnt)
    ctx = afv.Context()
    table = tbl.DescriptorTable(ctx, K, t.shape[1])
    fvs = []
    for k in range(K):
        table.set(k, t[k, :cnt[k]], ang[k, :cnt[k]])
        fv = _featvec(afv, 50 + k, int(cnt[k]), 40 if k % 3 else 7)
        fvs.append(fv)
        table.set_featvec(k, *_csr(fv))
    pa = np.array([k for k in range(K) for _ in range(3)], np.int32)
    pb = np.array([(k + 1 + j) % K for k in range(K) for j in range(3)], np.int32)
    # map-point validity masks on every third keyframe (FeatureMatcher.cc:593-597, :609-613): they change the greedy walk
    valid = [None] * K
    for k in range(0, K, 3):
        valid[k] = (afv.synth.lcg_bytes(700 + k, max(int(cnt[k]), 1))[:cnt[k]] > 60).astype(np.uint8)
        table.set_valid(k, valid[k])
    m, nm = table.match_bow(pa, pb, TH, RATIO, ori)
    total = 0
    for p in range(len(pa)):
        a, b = int(pa[p]), int(pb[p])
        want, wn = oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], fvs[a], fvs[b], valid[a], valid[b], ang[a, :cnt[a]], ang[b, :cnt[b]], TH, RATIO, ori)
        assert nm[p] == wn, (p, a, b)
        assert np.array_equal(m[p, :cnt[a]], want), (p, a, b)
        assert np.all(m[p, cnt[a]:] == -1)
        total += wn
    assert total > 50
    # counts-only call
    _, nm2 = table.match_bow(pa, pb, TH, RATIO, ori, want_matches=False)
    assert np.array_equal(nm, nm2)
    table.close()
    ctx.close()


@pytest.mark.parametrize("ori", [False, True])
def test_table_bow_frame_relocalisation_batch(afv, oracle, tbl, ori):
    """SearchByBoW(KF, Frame) (FeatureMatcher.cc:186-283) of ONE frame against 36 candidate keyframes of the table in one call
    (Tracking::Relocalization, Tracking.cc:1162,1182): ragged counts, an empty keyframe, validity masks on the keyframe side, the
    inclusive threshold, the rotation histogram keyed by the frame feature"""
    t, ang, cnt = _small_table(afv, K=36, cap=384)
    K = len(cnt)
    ctx = afv.Context()
    table = tbl.DescriptorTable(ctx, K, t.shape[1])
    fvs, valid = [], [None] * K
    for k in range(K):
        table.set(k, t[k, :cnt[k]], ang[k, :cnt[k]])
        # the same feature index sits in the same node in every keyframe (rows keep their identity along the table): real matches
        fv = _featvec(afv, 77, int(cnt[k]), 40 if k % 4 else 9)
        fvs.append(fv)
        table.set_featvec(k, *_csr(fv))
        if k % 3 == 0 and cnt[k]:
            valid[k] = (afv.synth.lcg_bytes(900 + k, int(cnt[k])) > 50).astype(np.uint8)
            table.set_valid(k, valid[k])
    # the frame: keyframe 17 seen again (10 % bit flips, 30 % new rows), 350 features, its own FeatureVector and angles
    nf = 350
    fdesc = afv.synth.perturbed_descriptors(t[17, :nf].copy(), 4242)
    fang = ((ang[17, :nf] + 3.0) % 360.0).astype(np.float32)
    ffv = _featvec(afv, 77, nf, 40)
    frame = afv.FeatureView(fdesc, ffv, None, fang)
    slots = np.array([k for k in range(K)][::-1], np.int32)           # every keyframe, the empty one included, in a non-trivial order
    m, nm = table.match_bow_frame(slots, frame, TH, RATIO, ori)
    assert m.shape == (K, nf)
    total = 0
    for p, k in enumerate(slots):
        want, wn = oracle.search_by_bow_kf_frame(t[k, :cnt[k]], fdesc, fvs[k], ffv, valid[k], ang[k, :cnt[k]], fang, TH, RATIO, ori)
        assert nm[p] == wn, (p, k)
        assert np.array_equal(m[p], want), (p, k)
        total += wn
    assert total > 300 and nm[list(slots).index(17)] > 100
    _, nm2 = table.match_bow_frame(slots, frame, TH, RATIO, ori, want_matches=False)
    assert np.array_equal(nm, nm2)
    # a frame without a FeatureVector shares no node with anybody; an empty frame is legal
    m0, nm0 = table.match_bow_frame(slots[:3], afv.FeatureView(fdesc, [], None, fang), TH, RATIO, ori)
    assert np.all(nm0 == 0) and np.all(m0 == -1)
    m1, nm1 = table.match_bow_frame(slots[:3], afv.FeatureView(np.zeros((0, 32), np.uint8), [], None, np.zeros(0, np.float32)), TH, RATIO, ori)
    assert np.all(nm1 == 0) and m1.shape == (3, 0)
    # a recycled slot without a FeatureVector must be refused, not answered with "no matches"
    table.set(2, t[2, :cnt[2]], ang[2, :cnt[2]])
    with pytest.raises(afv._lib.AfvError):
        table.match_bow_frame(np.array([2], np.int32), frame, TH, RATIO, ori)
    table.close()
    ctx.close()


def test_table_triangulation_pairs(afv, oracle, tbl):
    """device-resident SearchForTriangulation (FeatureMatcher.cc:662-790): per-keyframe geometry in the table, per pair only
    F12 / epipole / map-point masks"""
    s = afv.synth
    host = _small_table(afv, K=12, cap=320)
    t, ang, cnt = host
    K, cap = len(cnt), t.shape[1]
    ctx = afv.Context()
    table = tbl.DescriptorTable(ctx, K, cap)
    fvs, geo = [], []
    # geometry that is consistent with the table: row i is the same feature in every keyframe unless it was replaced, so it
    # keeps its image position up to a horizontal camera motion of 2 px per keyframe and half a pixel of vertical jitter
    x0 = (s.lcg_states(300, cap) % 60000).astype(np.float32) / 100.0
    y0 = (s.lcg_states(400, cap) % 47000).astype(np.float32) / 100.0
    oct_ = s.lcg_states(500, cap) % 8
    sg0 = ((np.float32(1.2) ** oct_.astype(np.float32)) ** 2).astype(np.float32)
    for k in range(K):
        n = int(cnt[k])
        table.set(k, t[k, :n], ang[k, :n])
        fv = _featvec(afv, 90, n, 25)              # same word for the same row: what a vocabulary does for near-identical descriptors
        fvs.append(fv)
        table.set_featvec(k, *_csr(fv))
        x = x0[:n] + np.float32(2 * k)
        y = y0[:n] + ((s.lcg_states(600 + k, max(n, 1))[:n] % 101).astype(np.float32) - 50) / np.float32(100.0)
        geo.append((x, y, sg0[:n].copy()))
        table.set_geometry(k, x, y, sg0[:n])
    pa = np.arange(K, dtype=np.int32)
    pb = ((pa + 1) % K).astype(np.int32)
    F = np.zeros((K, 9), np.float32)
    ep = np.zeros((K, 2), np.float32)
    mp1, mp2 = [], []
    for p in range(K):
        # pure horizontal translation: epipolar lines y2 = y1 (+ a small tilt per pair), epipole far outside the image
        tilt = (float(s.lcg_states(700 + p, 1)[0] % 21) - 10) * 1e-4
        F[p] = np.array([0, 0, 0, 0, 0, -1, tilt, 1, 0], np.float32)
        ep[p] = (1.0e6, 240.0) if p % 4 else (float(x0[3]) + 2 * int(pb[p]), float(y0[3]))   # every 4th pair: epipole ON a feature
        mp1.append((s.lcg_bytes(900 + p, max(int(cnt[pa[p]]), 1))[:cnt[pa[p]]] > 200).astype(np.uint8) if p % 2 else None)
        mp2.append((s.lcg_bytes(950 + p, max(int(cnt[pb[p]]), 1))[:cnt[pb[p]]] > 200).astype(np.uint8) if p % 3 else None)
    m, nm = table.match_triangulation(pa, pb, F, ep, TH, mp1, mp2)
    total = 0
    for p in range(K):
        a, b = int(pa[p]), int(pb[p])
        na, nb = int(cnt[a]), int(cnt[b])
        pts1 = np.stack([geo[a][0], geo[a][1]], 1) if na else np.zeros((0, 2), np.float32)
        pts2 = np.stack([geo[b][0], geo[b][1]], 1) if nb else np.zeros((0, 2), np.float32)
        want, wn = oracle.search_for_triangulation(t[a, :na], t[b, :nb], pts1, pts2, geo[b][2], F[p].reshape(3, 3), ep[p], fvs[a], fvs[b], mp1[p], mp2[p], TH)
        got = m[p, :na]
        if isinstance(want, np.ndarray) and want.ndim == 2:      # list of (idx1, idx2) pairs
            vec = np.full(na, -1, np.int32)
            for i1, i2 in want:
                vec[i1] = i2
            want = vec
        assert nm[p] == wn, (p, nm[p], wn)
        assert np.array_equal(got, np.asarray(want)[:na]), p
        total += wn
    assert total > 300
    # stereo keyframes (FeatureMatcher.cc:705-709, :727-731, :741): every second slot gets mvuRight for about half of its features; the
    # epipole-on-a-feature pairs then only lose their mono-mono candidates, and bOnlyStereo leaves the stereo-stereo ones
    urs = []
    for k in range(K):
        n = int(cnt[k])
        ur = None
        if k % 2 == 0 and n:
            ur = np.where(s.lcg_bytes(1000 + k, n) > 120, geo[k][0] - np.float32(11.0), np.float32(-1.0)).astype(np.float32)
        urs.append(ur)
        table.set_geometry(k, *geo[k], u_right=ur)
    changed = 0
    for only in (False, True):
        m2, nm2 = table.match_triangulation(pa, pb, F, ep, TH, mp1, mp2, only_stereo=only)
        for p in range(K):
            a, b = int(pa[p]), int(pb[p])
            na, nb = int(cnt[a]), int(cnt[b])
            pts1 = np.stack([geo[a][0], geo[a][1]], 1) if na else np.zeros((0, 2), np.float32)
            pts2 = np.stack([geo[b][0], geo[b][1]], 1) if nb else np.zeros((0, 2), np.float32)
            want, wn = oracle.search_for_triangulation(t[a, :na], t[b, :nb], pts1, pts2, geo[b][2], F[p].reshape(3, 3), ep[p], fvs[a], fvs[b],
                                                       mp1[p], mp2[p], TH, u_right1=urs[a], u_right2=urs[b], only_stereo=only)
            assert nm2[p] == wn, (only, p, nm2[p], wn)
            assert np.array_equal(m2[p, :na], np.asarray(want)[:na]), (only, p)
            changed += int(not np.array_equal(m2[p, :na], m[p, :na]))
    assert changed > 0  # the stereo branches changed some pair's outcome
    table.close()
    ctx.close()


def _replica_fixture(afv, tbl, ctx, K=10, cap=256):
    """a table with everything a replica has to carry: ragged counts, FeatureVectors, geometry, validity masks"""
    s = afv.synth
    t, ang, cnt = _small_table(afv, K=K, cap=cap)
    table = tbl.DescriptorTable(ctx, K, cap)
    x0 = (s.lcg_states(301, cap) % 60000).astype(np.float32) / 100.0
    y0 = (s.lcg_states(401, cap) % 47000).astype(np.float32) / 100.0
    sg0 = ((np.float32(1.2) ** (s.lcg_states(501, cap) % 8).astype(np.float32)) ** 2).astype(np.float32)
    fvs, geo, valid = [], [], [None] * K
    for k in range(K):
        n = int(cnt[k])
        table.set(k, t[k, :n], ang[k, :n])
        fv = _featvec(afv, 91, n, 25)
        fvs.append(fv)
        table.set_featvec(k, *_csr(fv))
        g = (x0[:n] + np.float32(2 * k), y0[:n].copy(), sg0[:n].copy())
        geo.append(g)
        table.set_geometry(k, *g)
        if k % 3 == 0:
            valid[k] = (s.lcg_bytes(710 + k, max(n, 1))[:n] > 60).astype(np.uint8)
            table.set_valid(k, valid[k])
    return table, (t, ang, cnt), fvs, geo, valid


def _replica_jobs(afv, K, cnt):
    s = afv.synth
    pa = np.array([k for k in range(K) for _ in range(2)], np.int32)
    pb = np.array([(k + 1 + j) % K for k in range(K) for j in range(2)], np.int32)
    F = np.tile(np.array([0, 0, 0, 0, 0, -1, 1e-4, 1, 0], np.float32), (len(pa), 1))
    ep = np.tile(np.array([1.0e6, 240.0], np.float32), (len(pa), 1))
    mp1 = [(s.lcg_bytes(905 + p, max(int(cnt[pa[p]]), 1))[:cnt[pa[p]]] > 200).astype(np.uint8) if p % 2 else None for p in range(len(pa))]
    return pa, pb, F, ep, mp1


def test_replica_answers_like_the_original(afv, oracle, tbl):
    """afv_table_clone rebuilds a second table (on another context) through the replica image + rebuild step that every receiver
    of afv_table_broadcast runs (LoopClosing.cc:255-281: the loop search on a non-root rank is BoW-guided too).  A table that was
    populated ONLY that way must answer the BoW-guided and triangulation batches exactly like the original — and like the oracle."""
    ctx_a, ctx_b = afv.Context(), afv.Context()
    table, (t, ang, cnt), fvs, geo, valid = _replica_fixture(afv, tbl, ctx_a)
    K, cap = len(cnt), t.shape[1]
    replica = tbl.DescriptorTable(ctx_b, K, cap)
    replica.set(0, t[1, :50], ang[1, :50])                     # previous content of the receiver must not survive
    replica.set_featvec(0, *_csr(_featvec(afv, 5, 50, 7)))
    table.clone_into(replica)
    pa, pb, F, ep, mp1 = _replica_jobs(afv, K, cnt)
    for ori in (False, True):
        m0, n0 = table.match_bow(pa, pb, TH, RATIO, ori)
        m1, n1 = replica.match_bow(pa, pb, TH, RATIO, ori)
        assert np.array_equal(n0, n1) and np.array_equal(m0, m1)
    assert n1.sum() > 50
    for p in range(0, len(pa), 3):
        a, b = int(pa[p]), int(pb[p])
        want, wn = oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], fvs[a], fvs[b], valid[a], valid[b], ang[a, :cnt[a]], ang[b, :cnt[b]],
                                              TH, RATIO, True)
        assert n1[p] == wn and np.array_equal(m1[p, :cnt[a]], want), p
    t0 = table.match_triangulation(pa, pb, F, ep, TH, mp1, None)
    t1 = replica.match_triangulation(pa, pb, F, ep, TH, mp1, None)
    assert np.array_equal(t0[1], t1[1]) and np.array_equal(t0[0], t1[0]) and t1[1].sum() > 100
    bp = replica.match_pairs(pa, pb, TH, RATIO, True)
    assert np.array_equal(bp[1], table.match_pairs(pa, pb, TH, RATIO, True)[1])
    replica.close(); table.close(); ctx_b.close(); ctx_a.close()


def test_recycled_slot_and_shrunk_counts(afv, tbl):
    """afv_table_set on a used slot forgets the slot's FeatureVector / geometry / validity mask, and a count that shrinks under a stored
    FeatureVector (afv_table_sync_counts after an external write of d_n) drops it: the guided batches then refuse the slot
    (AFV_EINVAL) instead of answering "no matches" or indexing rows that no longer exist"""
    import torch
    ctx = afv.Context()
    table, (t, ang, cnt), fvs, geo, valid = _replica_fixture(afv, tbl, ctx, K=6, cap=128)
    pa, pb = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    _, nm = table.match_bow(pa, pb, TH, RATIO, True)
    table.set(1, t[3, :100], ang[3, :100])                       # slot 1 recycled for another keyframe
    with pytest.raises(Exception):
        table.match_bow(pa, pb, TH, RATIO, True)
    table.set_featvec(1, *_csr(_featvec(afv, 91, 100, 25)))
    table.match_bow(pa, pb, TH, RATIO, True)                     # FeatureVector back: served again
    with pytest.raises(Exception):                               # ... but its geometry is still the old keyframe's
        table.match_triangulation(pa, pb, np.tile(np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32), (2, 1)),
                                  np.tile(np.array([1e6, 240.0], np.float32), (2, 1)), TH)
    # validity row of the recycled slot is "all valid" again: same answer as a fresh table holding the same data
    fresh = tbl.DescriptorTable(ctx, 6, 128)
    for k in range(6):
        src = 3 if k == 1 else k
        n = 100 if k == 1 else int(cnt[k])
        fresh.set(k, t[src, :n], ang[src, :n])
        fresh.set_featvec(k, *_csr(_featvec(afv, 91, n, 25)))
        if k % 3 == 0:
            fresh.set_valid(k, valid[k])
    a1, b1 = np.array([1, 2], np.int32), np.array([2, 1], np.int32)
    r0, r1 = table.match_bow(a1, b1, TH, RATIO, True), fresh.match_bow(a1, b1, TH, RATIO, True)
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
    # shrink slot 2 behind the library's back
    d, a, n = table.device_views()
    n[2] = 10
    torch.cuda.synchronize()
    table.sync_counts()
    with pytest.raises(Exception):
        table.match_bow(a1, b1, TH, RATIO, True)
    fresh.close(); table.close(); ctx.close()


def test_comm_world1_broadcast_and_allgather(afv, tbl):
    """the C-ABI communicator on a single rank: RCCL is found at run time, a world-1 broadcast / all-gather are identities and
    the table broadcast reports its device time.  (A 2-rank run needs 2 GPUs: see test_comm_two_ranks.)"""
    import torch
    ctx = afv.Context()
    comm = tbl.Communicator(ctx, 0, 1, lambda ident: ident)
    host = _small_table(afv, K=6, cap=128)
    table = tbl.DescriptorTable(ctx, 6, 128)
    table.upload(*host)
    ms = table.broadcast(comm, root=0)
    assert ms >= 0.0
    d, a, n = table.device_views()
    assert np.array_equal(d.cpu().numpy(), host[0]) and np.array_equal(n.cpu().numpy(), host[2])
    x = torch.arange(1000, dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    torch.cuda.synchronize()          # the collectives run on the context's own stream (stream = NULL)
    comm.broadcast(x)
    comm.allgather(x, y)
    torch.cuda.synchronize()
    assert afv._lib.load().afv_comm_rank(comm.handle) == 0 and afv._lib.load().afv_comm_size(comm.handle) == 1
    assert torch.equal(x, y)
    comm.close()
    table.close()
    ctx.close()


def _free_port():
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
    dist.init_process_group("gloo", rank=rank, world_size=world)   # host channel for the id only; the data path is RCCL in the library
    afv = importlib.import_module("anyfeature-vslam_amd")
    tbl = importlib.import_module("anyfeature-vslam_amd.table")
    dmod = importlib.import_module("anyfeature-vslam_amd.dist")

    def exchange(ident):
        box = [ident]
        dist.broadcast_object_list(box, src=0)
        return box[0]
    ctx = afv.Context(device=rank)
    comm = tbl.Communicator(ctx, rank, world, exchange)
    K, cap, njobs = 16, 256, 101
    host = afv.synth.keyframe_table(K, cap, seed=9)
    table = tbl.DescriptorTable(ctx, K, cap)
    if rank == 0:
        table.upload(*host)
    table.broadcast(comm, root=0)
    a, b = dmod.lcg_pairs(4, njobs, K)
    b = ((a.astype(np.int64) + 1 + (b.astype(np.int64) % 3)) % K).astype(np.int32)
    lo, hi = tbl.shard_range(njobs, rank, world)
    _, nm = table.match_pairs(a[lo:hi], b[lo:hi], TH, RATIO, True, want_matches=False)
    # the BoW-guided loop search on every rank's replica: only rank 0 ever called set_featvec / set_geometry
    rtab = tbl.DescriptorTable(ctx, 10, 256)
    if rank == 0:
        rtab.close()
        rtab, _, _, _, _ = _replica_fixture(afv, tbl, ctx)
    rtab.broadcast(comm, root=0)
    t_, ang_, cnt_ = _small_table(afv, K=10, cap=256)
    pa2, pb2, F2, ep2, mp12 = _replica_jobs(afv, 10, cnt_)
    bow = rtab.match_bow(pa2, pb2, TH, RATIO, True)
    tri = rtab.match_triangulation(pa2, pb2, F2, ep2, TH, mp12, None)
    q.put(("guided", rank, bow[0].tobytes(), bow[1].tolist(), tri[0].tobytes(), tri[1].tolist()))
    rtab.close()
    pad = tbl.shard_range(njobs, 0, world)[1]
    send = torch.full((pad,), -1, dtype=torch.int32, device="cuda")
    send[:hi - lo] = torch.from_numpy(nm).cuda()
    recv = torch.empty((pad * world,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    comm.allgather(send, recv)
    torch.cuda.synchronize()          # device-wide: covers the context's stream the collective ran on
    r = recv.cpu().numpy().reshape(world, pad)
    allnm = np.concatenate([r[k, :tbl.shard_range(njobs, k, world)[1] - tbl.shard_range(njobs, k, world)[0]] for k in range(world)])
    q.put((rank, allnm.tolist()))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_comm_two_ranks(afv, oracle):
    """2-rank RCCL run of the config-#4 exchange through the C-ABI: broadcast of the table, sharded jobs, all-gather of the
    counts.  Needs two GPUs (the round-end box has one: skipped there)."""
    import torch
    import torch.multiprocessing as mp
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    dmod = importlib.import_module("anyfeature-vslam_amd.dist")
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    msgs = [q.get(timeout=500) for _ in range(4)]
    guided = sorted((m for m in msgs if m[0] == "guided"), key=lambda m: m[1])
    assert guided[0][2:] == guided[1][2:] and sum(guided[1][3]) > 50 and sum(guided[1][5]) > 100   # the replica answers like the root
    res = sorted(m for m in msgs if m[0] != "guided")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    K, cap, njobs = 16, 256, 101
    host = afv.synth.keyframe_table(K, cap, seed=9)
    a, b = dmod.lcg_pairs(4, njobs, K)
    b = ((a.astype(np.int64) + 1 + (b.astype(np.int64) % 3)) % K).astype(np.int32)
    want = [_oracle_job(oracle, host, int(a[j]), int(b[j]))[1] for j in range(njobs)]
    assert res[0][1] == want and res[1][1] == want


@pytest.mark.timeout(600)
@pytest.mark.parametrize("workload", ["orb32", "pairs10k"])
def test_bench_two_ranks_on_one_device_through_the_self_launch(workload):
    """the N > 1 path of bench.py end to end, as far as one GPU allows: `python bench.py --gpus 2` without a launcher re-executes itself
    under torch.distributed.run (one process per rank, 127.0.0.1), both ranks share cuda:0 (--single-device) and talk gloo.  Checked on
    the JSON line: world size, per-rank ownership (frame seeds / job ranges), totals, and which replication path the table took."""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--single-device", "--steps", "2", "--warmup", "1",
           "--full", "--cpu-frames", "0", "--no-extras", "--no-profile", "--workload", workload]
    cmd += ["--batch", "16"] if workload == "orb32" else ["--keyframes", "64", "--jobs", "400", "--bcast-reps", "1"]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["steps"] == 2
    # the self-verification block of a multi-rank run: both layers saw two ranks, every rank names its device (here the same one)
    mg = d["multi_gpu"]
    assert mg["world_size"] == 2 and mg["backend"] == "gloo" and mg["rccl_ranks_seen"]["torch_distributed"] == 2
    assert [r["rank"] for r in mg["ranks"]] == [0, 1] and all(r["device_ordinal"] == 0 and r["device_name"] for r in mg["ranks"])
    assert mg["single_device_rehearsal"] is True and mg["distinct_devices"] == 1 and mg["one_rank_per_device"] is False
    assert "rccl_version" in mg and len({r["pid"] for r in mg["ranks"]}) == 2
    if workload == "orb32":
        pr = d["config"]["per_rank"]
        assert [p["rank"] for p in pr] == [0, 1] and [p["first_seed"] for p in pr] == [1, 17] and all(p["frames"] == 16 for p in pr)
        assert all(p["keypoints_per_step"] > 16 * 900 for p in pr) and pr[0]["keypoints_per_step"] != pr[1]["keypoints_per_step"]
        assert d["config"]["global_frames_per_step"] == 32 and d["scaling"] == "weak" and d["config"]["backend"] == "gloo"
        assert abs(d["value"] - sum(p["keypoints_per_step"] for p in pr) * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    else:
        assert d["config"]["job_ranges"] == [[0, 200], [200, 400]] and d["config"]["jobs_per_step"] == 400 and d["scaling"] == "strong"
        assert d["broadcast"]["bytes"] == 64 * 1000 * 32 + 64 * 1000 * 4 + 64 * 4
        assert d["broadcast"]["via"] == "torch.distributed.broadcast (gloo)"      # nccl: "afv_table_broadcast (ncclBroadcast ...)"
        # (with K = 64 the LCG pairs are all 16 keyframes apart - no overlap; the co-visible jobs b = a + 1..3 carry the matches)
        assert d["covisible"]["matches_per_job"] > 100

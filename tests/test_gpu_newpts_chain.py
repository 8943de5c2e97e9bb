"""-m gpu: afv_table_create_new_points - the neighbour loop of CreateNewMapPoints in one call, the masks kept on the device - against the
composed restatement (tests/_tri_ref.py over tests/_bow_ref.py) and against the existing neighbour-by-neighbour loop
(DescriptorTable.CreateNewMapPoints) on the scenes of tests/_newpts_scenes.py: observation lists, masks, ids and outputs exactly, x3D and
every field of the store as bits.  tests/test_newpts_ref_cpu.py proves on the CPU that the scenes exercise the chain."""
import ctypes as C

import numpy as np
import pytest

import _newpts_scenes as N
import _tri_ref as R
from test_gpu_triangulate import FIELDS, assert_store, bits, fill_slot, prefilled_store

pytestmark = pytest.mark.gpu
CAPS = {(1, 3, 40, 32, 0): 64, (2, 7, 70, 32, 0): 96, (3, 20, 130, 32, 0): 160, (5, 3, 257, 32, 0): 320, (6, 4, 64, 61, 0): 64, (7, 3, 48, 0, 128): 64}
ROW_IDS = lambda k: "seed%d-nn%d-n%d-%s" % (k[0], k[1], k[2], "f%d" % k[4] if k[4] else "b%d" % k[3])


def build_table(afv, ctx, ch, cap, skip=(), scale_less=()):
    kw = {"float_dim": ch.float_dim} if ch.float_dim else {"desc_bytes": ch.desc_bytes}
    t = afv.table.DescriptorTable(ctx, ch.nn + 1, cap, **kw)
    for k in range(ch.nn + 1):
        if k not in skip:
            fill_slot(t, k, ch.W.kfs[k], ch.W.desc[k], scale=k not in scale_less, featvec=True)
    return t


def store_for(afv, ctx, ch, capacity=300):
    return prefilled_store(afv, ctx, capacity, ch.desc_bytes, ch.float_dim)


def call_args(ch):
    W = ch.W
    return list(range(1, ch.nn + 1)), {k: W.cams[k] for k in range(ch.nn + 1)}, np.stack(W.F12), np.stack(W.epipoles)


def mask_dict(ch, cur=None, nb=None):
    c, n = ch.masks()
    cur, nb = (c if cur is None else cur.copy()), (n if nb is None else [m.copy() for m in nb])
    return dict([(0, cur)] + [(k + 1, nb[k]) for k in range(ch.nn)])


def padded_masks(ch, cap, cur=None, nb=None):
    d = mask_dict(ch, cur, nb)
    m_cur, m_nb = np.zeros(cap, np.uint8), np.zeros((ch.nn, cap), np.uint8)
    m_cur[:ch.n] = d[0]
    for k in range(ch.nn):
        m_nb[k, :ch.n] = d[k + 1]
    return m_cur, m_nb


def observations(want):
    return [(nid, [(0, i), (k + 1, j)]) for nid, k, i, j, _ in want]


def assert_masks(ch, has_mp, want, start=None, name=""):
    cur, nb = ch.final_masks(want, start)
    assert np.array_equal(has_mp[0], cur), (name, "mask of the current keyframe")
    for k in range(ch.nn):
        assert np.array_equal(has_mp[k + 1], nb[k]), (name, "mask of neighbour", k)


def raw(afv, t, ch, cap, points=None, first_id=None, masks=None, neighbours=None, only_stereo=False):
    nbs, cams, F12, ep = call_args(ch)
    nbs = nbs if neighbours is None else neighbours
    jobs = t.tri_points_jobs([cams[0]] * ch.nn, [cams[k + 1] for k in range(ch.nn)], cams[0]["ratio_factor"], cams[0]["max_size"])
    m_cur, m_nb = padded_masks(ch, cap) if masks is None else masks
    out = t.create_new_points(0, nbs, F12, ep, ch.th_low, jobs, m_cur, m_nb, points, ch.first_id if first_id is None else first_id, only_stereo)
    return out, m_cur, m_nb


# ---- 1. the rows of the table ----
@pytest.mark.parametrize("key", sorted(N.ROWS), ids=ROW_IDS)
def test_rows_equal_the_restatement_and_the_existing_loop(afv, gpu_ctx, key):
    ch = N.chain(*key)
    cap = CAPS[key]
    assert cap >= ch.n and ch.per_neighbour() == N.ROWS[key][0]
    nbs, cams, F12, ep = call_args(ch)
    pts, before = store_for(afv, gpu_ctx, ch)
    loop_pts, _ = store_for(afv, gpu_ctx, ch)
    t = t2 = None
    try:
        t, t2 = build_table(afv, gpu_ctx, ch, cap), build_table(afv, gpu_ctx, ch, cap)
        has_mp, loop_mp = mask_dict(ch), mask_dict(ch)
        got = t.CreateNewMapPointsChain(pts, 0, nbs, cams, F12, ep, ch.th_low, has_mp, ch.first_id)
        assert got == observations(ch.want), key
        assert_masks(ch, has_mp, ch.want, name=key)
        assert_store(pts, before, [(nid, k, i, f) for nid, k, i, j, f in ch.want], lambda p, i: ch.W.desc[0][i], key)
        loop = t2.CreateNewMapPoints(loop_pts, 0, nbs, cams, F12, ep, ch.th_low, loop_mp, ch.first_id)   # the yardstick
        assert got == loop
        assert all(np.array_equal(has_mp[k], loop_mp[k]) for k in has_mp)
        ids = np.arange(pts.capacity, dtype=np.int32)
        a, b = pts.get(ids), loop_pts.get(ids)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        if key[2] == 257:   # features 255 and 256 sit in different workgroups: ranks and ids cross that edge
            lo = [nid for nid, k, i, j, _ in ch.want if k == 1 and i <= 255]
            hi = [nid for nid, k, i, j, _ in ch.want if k == 1 and i >= 256]
            assert lo and hi and min(hi) == max(lo) + 1
    finally:
        pts.close(); loop_pts.close()
        for x in (t, t2):
            if x is not None:
                x.close()


# ---- 2. the raw outputs, neighbour by neighbour ----
@pytest.mark.parametrize("key", [(2, 7, 70, 32, 0), (5, 3, 257, 32, 0), (7, 3, 48, 0, 128)], ids=ROW_IDS)
def test_raw_outputs_equal_the_two_calls_of_the_loop(afv, gpu_ctx, key):
    ch = N.chain(*key)
    cap = CAPS[key]
    nbs, cams, F12, ep = call_args(ch)
    pts, _ = store_for(afv, gpu_ctx, ch)
    loop_pts, _ = store_for(afv, gpu_ctx, ch)
    t = t2 = None
    try:
        t, t2 = build_table(afv, gpu_ctx, ch, cap), build_table(afv, gpu_ctx, ch, cap)
        (m, status, route, x3d, new_id, n_new, n_done), m_cur, m_nb = raw(afv, t, ch, cap, pts)
        assert n_done == ch.nn and tuple(n_new.tolist()) == N.ROWS[key][0]
        masks = mask_dict(ch)
        nid = ch.first_id
        for k, nb in enumerate(nbs):
            wm, _ = t2.match_triangulation([0], [nb], F12[k:k + 1], ep[k:k + 1], ch.th_low, [masks[0]], [masks[nb]])
            jobs = t2.tri_points_jobs([cams[0]], [cams[nb]], cams[0]["ratio_factor"], cams[0]["max_size"])
            ws, wr, wx, wid, wn = t2.triangulate([0], [nb], jobs, wm, loop_pts, nid)
            assert np.array_equal(m[k], wm[0]), (key, k, "match12")
            assert np.array_equal(status[k], ws[0]) and np.array_equal(route[k], wr[0]), (key, k, "status / route")
            assert np.array_equal(bits(x3d[k]), bits(wx[0])), (key, k, "x3d")
            assert np.array_equal(new_id[k], wid[0]) and n_new[k] == wn[0], (key, k, "ids")
            for i in np.nonzero(wid[0] >= 0)[0]:
                masks[0][i] = 1
                masks[nb][int(wm[0, i])] = 1
            nid += int(wn[0])
        assert np.array_equal(m_cur[:ch.n], masks[0]) and not m_cur[ch.n:].any()
        for k, nb in enumerate(nbs):
            assert np.array_equal(m_nb[k, :ch.n], masks[nb]) and not m_nb[k, ch.n:].any()
    finally:
        pts.close(); loop_pts.close()
        for x in (t, t2):
            if x is not None:
                x.close()


# ---- 3. the capacity rule ----
def test_a_store_that_ends_inside_neighbour_1(afv, gpu_ctx):
    key = (1, 3, 40, 32, 0)
    ch = N.chain(*key)
    assert N.ROWS[key][0] == (23, 11, 0)
    cap, L = CAPS[key], afv._lib
    nbs, cams, F12, ep = call_args(ch)
    capacity = ch.first_id + 23 + 10
    first = [w for w in ch.want if w[1] == 0]
    pts, before = store_for(afv, gpu_ctx, ch, capacity)
    loop_pts, _ = store_for(afv, gpu_ctx, ch, capacity)
    exact, exact_before = store_for(afv, gpu_ctx, ch, ch.first_id + 34)
    t = t2 = None
    try:
        t, t2 = build_table(afv, gpu_ctx, ch, cap), build_table(afv, gpu_ctx, ch, cap)
        (m, status, route, x3d, new_id, n_new, n_done), m_cur, m_nb = raw(afv, t, ch, cap, pts)
        assert n_done == 1 and n_new.tolist() == [23, 0, 0]
        assert (m[0] >= 0).sum() >= 23 and sorted(new_id[0][new_id[0] >= 0].tolist()) == list(range(ch.first_id, ch.first_id + 23))
        assert (m[1:] == -1).all() and not status[1:].any() and not route[1:].any() and not x3d[1:].any() and (new_id[1:] == -1).all()
        cur, nb = ch.final_masks(first)                                  # neighbour 0 stands, in the masks ...
        assert np.array_equal(m_cur[:ch.n], cur) and all(np.array_equal(m_nb[k, :ch.n], nb[k]) for k in range(ch.nn))
        # ... and in the store; no id at or beyond the capacity exists, every other id holds its prefill
        assert_store(pts, before, [(nid, k, i, f) for nid, k, i, j, f in first], lambda p, i: ch.W.desc[0][i], "capacity")
        # the method raises as the loop does, and the loop leaves the same state
        has_mp, loop_mp = mask_dict(ch), mask_dict(ch)
        again, _ = store_for(afv, gpu_ctx, ch, capacity)
        try:
            for fn, store, masks in ((t.CreateNewMapPointsChain, again, has_mp), (t2.CreateNewMapPoints, loop_pts, loop_mp)):
                with pytest.raises(L.AfvError) as e:
                    fn(store, 0, nbs, cams, F12, ep, ch.th_low, masks, ch.first_id)
                assert e.value.code == L.ECAPACITY
            assert all(np.array_equal(has_mp[k], loop_mp[k]) for k in has_mp) and np.array_equal(has_mp[0], cur)
            ids = np.arange(capacity, dtype=np.int32)
            a, b, c = pts.get(ids), loop_pts.get(ids), again.get(ids)
            assert all(a[k].tobytes() == b[k].tobytes() == c[k].tobytes() for k in a)
        finally:
            again.close()
        # a store that takes exactly the 34 points
        (_, _, _, _, new_id, n_new, n_done), m_cur, m_nb = raw(afv, t, ch, cap, exact)
        assert n_done == 3 and n_new.tolist() == [23, 11, 0] and int(new_id.max()) == exact.capacity - 1
        assert_store(exact, exact_before, [(nid, k, i, f) for nid, k, i, j, f in ch.want], lambda p, i: ch.W.desc[0][i], "exact capacity")
        # a first id beyond the store: nothing runs
        (m, _, _, _, new_id, n_new, n_done), m_cur, m_nb = raw(afv, t, ch, cap, exact, first_id=exact.capacity + 1)
        assert n_done == 0 and (m == -1).all() and (new_id == -1).all() and not n_new.any()
        assert np.array_equal(m_cur[:ch.n], ch.has_mp_cur)
    finally:
        pts.close(); loop_pts.close(); exact.close()
        for x in (t, t2):
            if x is not None:
                x.close()


# ---- 4. empty cases ----
def test_neighbours_without_matches_in_first_and_middle_position(afv, gpu_ctx):
    key = (2, 7, 70, 32, 0)
    ch = N.chain(*key)
    cap = CAPS[key]
    nbs, cams, F12, ep = call_args(ch)
    cur, nb = ch.masks()
    nb[0][:] = 1
    nb[2][:] = 1
    want = ch.restate(cur, nb)
    counts = ch.per_neighbour(want)
    assert counts[0] == 0 and counts[2] == 0 and counts[1] > 0 and sum(1 for c in counts[3:] if c > 0) >= 2
    pts, before = store_for(afv, gpu_ctx, ch)
    t = None
    try:
        t = build_table(afv, gpu_ctx, ch, cap)
        has_mp = mask_dict(ch, cur, nb)
        got = t.CreateNewMapPointsChain(pts, 0, nbs, cams, F12, ep, ch.th_low, has_mp, ch.first_id)
        assert got == observations(want)
        assert_masks(ch, has_mp, want, start=(cur, nb), name="empty neighbours")
        assert_store(pts, before, [(nid, k, i, f) for nid, k, i, j, f in want], lambda p, i: ch.W.desc[0][i], "empty neighbours")
    finally:
        pts.close()
        if t is not None:
            t.close()


def test_a_neighbour_slot_without_features_and_a_call_without_a_store(afv, gpu_ctx):
    key = (2, 7, 70, 32, 0)
    ch = N.chain(*key)
    cap = CAPS[key]
    nbs, cams, F12, ep = call_args(ch)
    pts, _ = store_for(afv, gpu_ctx, ch)
    loop_pts, _ = store_for(afv, gpu_ctx, ch)
    t = t2 = full = None
    try:
        t, t2 = build_table(afv, gpu_ctx, ch, cap, skip=(2,)), build_table(afv, gpu_ctx, ch, cap, skip=(2,))   # neighbour 1 = slot 2 is empty
        has_mp, loop_mp = mask_dict(ch), mask_dict(ch)
        got = t.CreateNewMapPointsChain(pts, 0, nbs, cams, F12, ep, ch.th_low, has_mp, ch.first_id)
        loop = t2.CreateNewMapPoints(loop_pts, 0, nbs, cams, F12, ep, ch.th_low, loop_mp, ch.first_id)
        assert got == loop and len(got) > 20 and not any(obs[1][0] == 2 for _, obs in got)
        assert [nid for nid, _ in got] == list(range(ch.first_id, ch.first_id + len(got)))
        assert all(np.array_equal(has_mp[k], loop_mp[k]) for k in has_mp)
        ids = np.arange(pts.capacity, dtype=np.int32)
        a, b = pts.get(ids), loop_pts.get(ids)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        # points=None: the same answers, nothing stored, no capacity rule
        full = build_table(afv, gpu_ctx, ch, cap)
        with_store, c1, n1 = raw(afv, full, ch, cap, pts)
        without, c2, n2 = raw(afv, full, ch, cap, None)
        assert with_store[6] == without[6] == ch.nn
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(with_store[:6], without[:6]))
        assert np.array_equal(c1, c2) and np.array_equal(n1, n2)
    finally:
        pts.close(); loop_pts.close()
        for x in (t, t2, full):
            if x is not None:
                x.close()


# ---- 5. validation: refused before any launch, masks and store as they were ----
def test_refusals_leave_masks_and_store_untouched(afv, gpu_ctx):
    key = (1, 3, 40, 32, 0)
    ch = N.chain(*key)
    cap, L = CAPS[key], afv._lib
    lib = L.load()
    nbs, cams, F12, ep = call_args(ch)
    pts, before = store_for(afv, gpu_ctx, ch)
    other_width = afv.MapPoints(gpu_ctx, 64, desc_bytes=61)
    t = bare = None

    def refused(table, expect, neighbours=nbs, points=pts, edit=None, null_mask=False, nn=None):
        nn = len(neighbours) if nn is None else nn
        n = max(nn, 1)
        search = (L.TableTriJob * n)()
        keep = np.ones(cap, np.uint8)
        for k in range(n):
            search[k].struct_size = C.sizeof(L.TableTriJob)
            search[k].th_low = ch.th_low
        if edit:
            edit(search, keep)
        jobs = table.tri_points_jobs([cams[0]] * n, [cams[1]] * n, cams[0]["ratio_factor"], cams[0]["max_size"])
        m_cur, m_nb = padded_masks(ch, cap)
        if nn > ch.nn:
            m_nb = np.zeros((nn, cap), np.uint8)
        c0, n0 = m_cur.copy(), m_nb.copy()
        arr = np.asarray(list(neighbours) + [0] * max(0, n - len(neighbours)), np.int32)
        n_new, n_done = np.zeros(n, np.int32), C.c_int32(-7)
        rc = lib.afv_table_create_new_points(table.handle, 0, L.ptr(arr), nn, search, jobs, None if null_mask else L.ptr(m_cur), L.ptr(m_nb),
                                             None if points is None else points.handle, ch.first_id, None, None, None, None, None, L.ptr(n_new),
                                             C.byref(n_done))
        assert rc == expect, (rc, expect)
        assert np.array_equal(m_cur, c0) and np.array_equal(m_nb, n0) and n_done.value == -7
        after = pts.get(np.arange(pts.capacity, dtype=np.int32))
        assert all(after[k].tobytes() == before[k].tobytes() for k in after)
    try:
        t = build_table(afv, gpu_ctx, ch, cap)
        bare = build_table(afv, gpu_ctx, ch, cap, scale_less=(2,))
        refused(t, L.EINVAL, nn=0)
        refused(t, L.EINVAL, neighbours=list(range(1, 66)))                                      # nn = 65
        refused(t, L.EINVAL, neighbours=[1, 0, 3])                                               # a neighbour equal to cur
        refused(t, L.EINVAL, neighbours=[1, 2, 1])                                               # a neighbour listed twice
        refused(t, L.EINVAL, neighbours=[1, 2, 9])                                               # a slot out of range
        refused(t, L.EINVAL, edit=lambda s, keep: setattr(s[1], "has_mp1", keep.ctypes.data))    # the masks do not travel in the records
        refused(t, L.EINVAL, edit=lambda s, keep: setattr(s[0], "has_mp2", keep.ctypes.data))
        refused(t, L.EINVAL, edit=lambda s, keep: setattr(s[2], "struct_size", 6))               # an unknown struct_size
        refused(t, L.EINVAL, null_mask=True)
        refused(bare, L.EINVAL)                                                                  # a slot without its scale planes
        refused(t, L.EUNSUPPORTED, points=other_width)                                           # a store of another width
        with pytest.raises(L.AfvError) as e:                                                     # ... and through the Python method
            raw(afv, t, ch, cap, pts, neighbours=[1, 2, 2])
        assert e.value.code == L.EINVAL
        (_, _, _, _, _, n_new, n_done), _, _ = raw(afv, t, ch, cap, pts)                          # the table still answers
        assert n_done == 3 and n_new.tolist() == [23, 11, 0]
    finally:
        pts.close(); other_width.close()
        for x in (t, bare):
            if x is not None:
                x.close()


# ---- 6. other slot sources ----
def test_a_current_keyframe_promoted_from_a_frame_and_a_cloned_table(afv, gpu_ctx):
    """slot 0 comes from afv_table_set_from_frame: its FeatureVector body is on the device only (the call fetches it for the row maps), its
    sigma2 is size^2, its scale planes are the frame's.  The table is then cloned and the clone answers alike."""
    ch = N.Chain(1, 3, 40)                     # an instance of its own: its current keyframe is replaced below
    a = ch.W.kfs[0]
    ch.W.kfs[0] = R.KF(a.x, a.y, a.size * a.size, a.size, u_right=np.full(a.n, -1, np.float32), depth=np.full(a.n, -1, np.float32), x_dist=a.x, y_dist=a.y)
    want = ch.want
    assert sum(1 for c in ch.per_neighbour() if c > 0) >= 2
    cap = 64
    nbs, cams, F12, ep = call_args(ch)
    rng = np.random.default_rng(5)
    # a vocabulary of two leaves; levelsup = L puts every feature into the root's node 0, the node of fill_slot's FeatureVector
    voc = afv.Vocabulary(2, 1, np.array([0, 0, 0], np.int32), rng.integers(0, 256, (3, 32), dtype=np.uint8), np.ones(3), np.array([0, 1, 1], bool), ctx=gpu_ctx)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=cap)
    pts, before = store_for(afv, gpu_ctx, ch)
    clone_pts, clone_before = store_for(afv, gpu_ctx, ch)
    t = dst = None
    try:
        kps = np.zeros(a.n, afv.KP_DTYPE)
        kps["x"], kps["y"] = a.x, a.y
        fr.set_features(kps, ch.W.desc[0], sizes=a.size)
        fr.ComputeBoW(voc, 1)
        assert fr.featvec() == [(0, list(range(a.n)))]
        t = build_table(afv, gpu_ctx, ch, cap, skip=(0,))
        t.set_from_frame(0, fr)
        dst = build_table(afv, gpu_ctx, ch, cap, skip=(0, 1, 2, 3))
        t.clone_into(dst)
        for table, store, prefill in ((t, pts, before), (dst, clone_pts, clone_before)):
            has_mp = mask_dict(ch)
            got = table.CreateNewMapPointsChain(store, 0, nbs, cams, F12, ep, ch.th_low, has_mp, ch.first_id)
            assert got == observations(want)
            assert_masks(ch, has_mp, want, name="promoted")
            assert_store(store, prefill, [(nid, k, i, f) for nid, k, i, j, f in want], lambda p, i: ch.W.desc[0][i], "promoted")
    finally:
        pts.close(); clone_pts.close(); fr.close(); voc.close()
        for x in (t, dst):
            if x is not None:
                x.close()


# ---- 7. repeatability ----
def test_the_same_call_twice_gives_the_same_outputs(afv, gpu_ctx):
    key = (3, 20, 130, 32, 0)
    ch = N.chain(*key)
    cap = CAPS[key]
    pts, _ = store_for(afv, gpu_ctx, ch)
    t = None
    try:
        t = build_table(afv, gpu_ctx, ch, cap)
        one, c1, n1 = raw(afv, t, ch, cap, pts)
        ids = np.arange(pts.capacity, dtype=np.int32)
        first = pts.get(ids)
        two, c2, n2 = raw(afv, t, ch, cap, pts)
        assert one[6] == two[6] == ch.nn and tuple(one[5].tolist()) == N.ROWS[key][0]
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(one[:6], two[:6]))
        assert np.array_equal(c1, c2) and np.array_equal(n1, n2)
        second = pts.get(ids)
        assert all(first[k].tobytes() == second[k].tobytes() for k in first)
    finally:
        pts.close()
        if t is not None:
            t.close()


# ---- 8. the points are in view ----
def test_search_local_points_sees_the_chains_points_without_an_upload(afv, gpu_ctx):
    """Frame.SearchLocalPoints on the ids just created, against the same search on a store filled with afv_points_set from the restatement"""
    key = (1, 3, 40, 32, 0)
    ch = N.chain(*key)
    W, want = ch.W, ch.want
    nbs, cams, F12, ep = call_args(ch)
    made, _ = prefilled_store(afv, gpu_ctx, 200)
    host, _ = prefilled_store(afv, gpu_ctx, 200)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=320)
    t = None
    try:
        t = build_table(afv, gpu_ctx, ch, CAPS[key])
        got = t.CreateNewMapPointsChain(made, 0, nbs, cams, F12, ep, ch.th_low, mask_dict(ch), ch.first_id)
        ids = np.array([nid for nid, _ in got], np.int32)
        assert len(ids) == 34
        f = [w[4] for w in want]
        host.set(ids, **{k: np.stack([x[k] for x in f]) for k in FIELDS})
        host.set_flags(ids, bad=np.zeros(len(ids)), observed=np.ones(len(ids)))
        host.set_descriptors(ids, np.stack([W.desc[0][i] for _, _, i, _, _ in want]))
        kf, cam = W.kfs[2], W.cams[2]
        kps = np.zeros(kf.n, afv.KP_DTYPE)
        kps["x"], kps["y"] = kf.x, kf.y
        fr.set_features(kps, W.desc[2], sizes=kf.size)
        fr.set_pose(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.0)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(100.0)
        try:
            m = afv.FeatureMatcher(0.8, False, ctx=gpu_ctx)
            a = fr.SearchLocalPoints(m, made, ids, 3.0)
            b = fr.SearchLocalPoints(m, host, ids, 3.0)
        finally:
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        assert a[1] == b[1] and a[1] > len(ids) // 2
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    finally:
        made.close(); host.close(); fr.close()
        if t is not None:
            t.close()

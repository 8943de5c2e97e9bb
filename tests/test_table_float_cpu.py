"""CPU: the entry point of float keyframe tables refuses bad arguments without a GPU, DescriptorTable's argument errors never reach the
library, and the data of tests/test_gpu_table_float.py reach the branches they are meant for - proven on the oracle alone."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FMAX = np.float32(3.4028235e38)


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("_table_float_gpu", os.path.join(HERE, "test_gpu_table_float.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_create_f32_refuses_bad_arguments(afv):
    lib = afv._lib.load()
    h = C.c_void_p()
    for dim in (128, 64, 4, 1024, 0, 3):      # null context: refused whatever the dimension
        assert lib.afv_table_create_f32(None, 4, 16, dim, C.byref(h)) == afv._lib.EINVAL
    assert lib.afv_table_create_f32(None, 4, 16, 128, None) == afv._lib.EINVAL
    # a dimension outside the rule (a multiple of 4 from 4 to 1024) is refused for its own sake, before the context is looked at: a
    # non-null stand-in that is no context (zeroed host memory, never dereferenced on this path) reaches no GPU
    dummy = C.create_string_buffer(4096)
    for dim in (0, 3, 6, 1028, -4):
        h = C.c_void_p()
        assert lib.afv_table_create_f32(C.cast(dummy, C.c_void_p), 4, 16, dim, C.byref(h)) == afv._lib.EINVAL
        assert h.value is None
    assert lib.afv_abi_version() == 6


class _NoLibrary:
    """a context whose library must not be touched"""

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    lib = _Lib()
    handle = None

    def check(self, *a, **k):
        raise AssertionError("the library was called")


def test_descriptor_table_argument_errors_never_reach_the_library(afv):
    tbl = importlib.import_module("anyfeature-vslam_amd.table")
    ctx = _NoLibrary()
    with pytest.raises(ValueError):
        tbl.DescriptorTable(ctx, 2, 16, desc_bytes=32, float_dim=128)
    with pytest.raises(ValueError):
        tbl.DescriptorTable(ctx, 2, 16, desc_bytes=64, float_dim=16)
    for bad in (0, 3, 6, 1028, -4, 128.0, True, "128"):
        with pytest.raises(ValueError):
            tbl.DescriptorTable(ctx, 2, 16, float_dim=bad)
    # row checks of a float table (an object that only carries the shape: no handle, no library)
    t = tbl.DescriptorTable.__new__(tbl.DescriptorTable)
    t.ctx, t.lib, t.nsets, t.cap, t.float_dim, t.desc_bytes, t.pitch, t.handle = ctx, ctx.lib, 2, 16, 64, 256, 256, None
    for bad in (np.zeros((4, 128), np.float32), np.zeros((4, 64), np.uint8), np.zeros((4, 256), np.uint8), np.zeros(256, np.float32),
                np.zeros((4, 64), np.float64)):
        with pytest.raises(ValueError):
            t.set(0, bad)
    for bad in (np.zeros((4, 128), np.float32), np.zeros((4, 64), np.uint8)):
        with pytest.raises(ValueError):
            t.match_bow_frame(np.array([0], np.int32), afv.FeatureView(bad), 1.0, 0.75)
    with pytest.raises(ValueError):
        t.upload(np.zeros((2, 16, 64), np.uint8), np.zeros((2, 16), np.float32), np.zeros(2, np.int32))


def _l2sqr_matrix(x, y):
    """cv::norm(a, b, NORM_L2SQR) for every (row, column): float differences, squares and the sum of each group of four in double
    (v0*v0 + v1*v1 + v2*v2 + v3*v3, left to right), the groups added in order, one narrowing to float at the end"""
    s = np.zeros((len(x), len(y)), np.float64)
    for g in range(0, x.shape[1], 4):
        v = (x[:, None, g:g + 4] - y[None, :, g:g + 4]).astype(np.float64)       # the subtraction is float32
        sq = v * v
        s += ((sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2]) + sq[:, :, 3]
    return s.astype(np.float32)


def _greedy_ref(dist, th, ratio):
    """SearchByBoW(KF,KF) brute force written directly from the rule: rows in order; among the columns not taken yet the best (ties to
    the earlier column) is accepted if best < th and best < ratio * second, the product in float"""
    n1, n2 = dist.shape
    taken = np.zeros(n2, bool)
    out = np.full(n1, -1, np.int32)
    th, ratio = np.float32(th), np.float32(ratio)
    for i in range(n1):
        if taken.all() or n2 == 0:
            continue
        d = np.where(taken, np.inf, dist[i].astype(np.float64))
        c = int(np.argmin(d))
        best = np.float32(d[c])
        d[c] = np.inf
        second = np.float32(d.min()) if np.isfinite(d.min()) else FMAX
        if best < th and best < np.float32(ratio * second):
            out[i] = c
            taken[c] = True
    return out, int((out >= 0).sum())


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("dim", [64, 128, 256, 36, 200])
def test_pair_data_reach_their_branches(afv, oracle, dim, real):
    mod = _gpu_test_module()
    rows, angles, th = mod.pair_data(afv, dim, real)
    a, b = rows[0], rows[1]
    dist = _l2sqr_matrix(a, b)
    # the numpy restatement of the rule agrees with the oracle (cv::norm's summation order included)
    for ratio in (0.75, 1.0):
        want, wn = oracle.search_by_bow_kf_kf(a, b, th_low=th, nnratio=ratio, check_orientation=False)
        got, n = _greedy_ref(dist, th, ratio)
        assert n == wn and np.array_equal(got, want), (dim, real, ratio)
    # ... on the ragged sets too
    got, n = _greedy_ref(_l2sqr_matrix(rows[5], rows[3]), th, 1.0)
    want, wn = oracle.search_by_bow_kf_kf(rows[5], rows[3], th_low=th, nnratio=1.0, check_orientation=False)
    assert n == wn and np.array_equal(got, want)
    # the rotation histogram removes matches
    off, noff = oracle.search_by_bow_kf_kf(a, b, angle1=angles[0], angle2=angles[1], th_low=th, nnratio=1.0, check_orientation=False)
    on, non = oracle.search_by_bow_kf_kf(a, b, angle1=angles[0], angle2=angles[1], th_low=th, nnratio=1.0, check_orientation=True)
    assert not np.array_equal(on, off) and 0 < non < noff, (dim, real)
    # a row matched to a column that is not among its 4 nearest by (distance, column): the 4-key list of phase 1 is used up and the
    # ordered phase rescans the row exactly
    order = np.lexsort((np.broadcast_to(np.arange(dist.shape[1]), dist.shape), dist), axis=1)[:, :4]
    beyond = sum(1 for i, c in enumerate(off) if c >= 0 and c not in order[i])
    if dim in (128, 256) and (real or dim == 128):
        assert beyond >= 1, (dim, real, beyond)
    if not real:
        two = np.sort(dist, axis=1)[:, :2]
        assert np.any(two[:, 0] == two[:, 1])         # equal best distances: the key order (distance, column) decides
        i = int(np.argmax(two[:, 0] == two[:, 1]))
        assert order[i, 0] < order[i, 1] and dist[i, order[i, 0]] == dist[i, order[i, 1]]


@pytest.mark.parametrize("dim", [64, 36, 256])
def test_guided_data_match(afv, oracle, dim):
    """the data of the BoW / triangulation tests produce matches on the oracle (the GPU test asserts the same totals)"""
    mod = _gpu_test_module()
    for real in (False, True):
        t32, t, ang, cnt, fvs, geo, valid = mod.guided_data(afv, dim, real)
        th = mod._th(dim, real)
        total = 0
        for a in range(8):
            b = (a + 1) % 8
            total += oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], fvs[a], fvs[b], valid[a], valid[b], ang[a, :cnt[a]],
                                                ang[b, :cnt[b]], th, 0.75, True)[1]
        assert total > 20, (dim, real)

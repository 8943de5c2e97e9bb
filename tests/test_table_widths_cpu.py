"""CPU: the entry point of tables wider or narrower than 32 bytes refuses bad arguments without a GPU, and the Hamming reference the GPU
test expects agrees with the oracle's brute force at widths 61 and 64 on the adversarial rows."""
import ctypes as C
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu_test_module():
    spec = importlib.util.spec_from_file_location("_table_widths_gpu", os.path.join(HERE, "test_gpu_table_widths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_create_bytes_refuses_bad_arguments(afv):
    lib = afv._lib.load()
    h = C.c_void_p()
    for w in (0, 65, 61, 32, 1, 64):      # null context: refused whatever the width
        assert lib.afv_table_create_bytes(None, 4, 16, w, C.byref(h)) == afv._lib.EINVAL
    assert lib.afv_table_create_bytes(None, 4, 16, 61, None) == afv._lib.EINVAL
    # a width outside 1..64 is refused for its own sake, before the context is looked at: a non-null stand-in that is no context
    # (zeroed host memory, never dereferenced on this path) reaches no GPU
    dummy = C.create_string_buffer(4096)
    for w in (0, 65, -1, 1000):
        h = C.c_void_p()
        assert lib.afv_table_create_bytes(C.cast(dummy, C.c_void_p), 4, 16, w, C.byref(h)) == afv._lib.EINVAL
        assert h.value is None


def _hamming_ref(x, y, th, ratio):
    """SearchByBoW(KF,KF) brute force written directly from the rule: greedy rows in order, best < th and best < ratio * second among the
    columns not taken yet, ties to the earlier column"""
    dist = np.unpackbits(x[:, None, :] ^ y[None, :, :], axis=2).sum(2)
    taken = np.zeros(len(y), bool)
    out = np.full(len(x), -1, np.int32)
    for i in range(len(x)):
        d = np.where(taken, 1 << 30, dist[i])
        order = np.argsort(d, kind="stable")
        best = d[order[0]] if len(order) else 1 << 30
        second = d[order[1]] if len(order) > 1 else 1 << 30
        if best < (1 << 30) and best < th and best < ratio * (second if second < (1 << 30) else np.inf):
            out[i] = order[0]
            taken[order[0]] = True
    return out, int((out >= 0).sum())


def test_numpy_reference_agrees_with_the_oracle(afv, oracle):
    mod = _gpu_test_module()
    for w in (61, 64):
        a, b = mod._adversarial(afv, w)
        th = mod._th(w)
        assert np.unpackbits(a[0] ^ b[0]).sum() == 8 * w
        for ratio in (0.75, 1.0):
            for x, y in ((a, b), (b, a)):
                want, wn = oracle.search_by_bow_kf_kf(x, y, th_low=th, nnratio=ratio, check_orientation=False)
                got, n = _hamming_ref(x, y, th, ratio)
                assert n == wn and np.array_equal(got, want), (w, ratio)

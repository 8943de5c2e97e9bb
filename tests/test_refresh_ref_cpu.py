"""CPU: the restatement tests/_refresh_ref.py on the constructed scenes of tests/_refresh_scenes.py - every point of rule_scene reaches the
rule it is named after, the restated median equals a sort - and tools/refresh_host.cpp, the scalar host program tools/time_refresh.py
times the device against, answers what the restatement answers, bit for bit.  The same source, built as the stand-alone program it also
is with -fsanitize=address,undefined, runs clean (no sanitizer touches code loaded into Python)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _refresh_ref as R
import _refresh_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "refresh_host.cpp")
FIELDS = ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma", "flags", "descriptors")


@functools.lru_cache(maxsize=None)
def rule_case(kind):
    sc = S.rule_scene(kind)
    return sc, R.refresh(sc)


def rules_of(kind):
    return list(S.RULES) + [r for r, k in S.ONLY.items() if k == kind or (k[1] is None and k[0] == kind[0])]


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def unchanged(before, after, keys):
    return all(same(before[k], after[k]) for k in keys)


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_every_point_reaches_its_rule(kind):
    sc, (status, best, med, store) = rule_case(kind)
    assert sorted(sc.rule) == sorted(rules_of(kind))
    at = {r: sc.point_ids.index(pid) for r, pid in sc.rule.items()}
    obs_of = lambda r: [e for e, o in enumerate(sc.observations) if o[0] == sc.rule[r]]
    st = lambda r: status[at[r]]
    chosen = lambda r: obs_of(r).index(best[at[r]]) if best[at[r]] >= 0 else -1
    normal_written = lambda r: not unchanged(sc.store[sc.rule[r]], store[sc.rule[r]], R.PLANES)
    row_written = lambda r: not same(sc.store[sc.rule[r]]["descriptors"], store[sc.rule[r]]["descriptors"])
    assert st("n1") == R.DONE and chosen("n1") == 0 and med[at["n1"]] == 0
    assert chosen("n2_identical_rows") == 0 and med[at["n2_identical_rows"]] == 0       # the median is the self-distance
    assert chosen("n3") == 1 and chosen("n4") == 1 and med[at["n4"]] > 0
    assert chosen("equal_medians") == 0 and med[at["equal_medians"]] > 0
    # the first, a middle and the last observation are of bad keyframes: the winner is counted in the whole list
    assert chosen("bad_kf_front") == 1 and chosen("bad_kf_middle") == 0 and chosen("bad_kf_end") == 0
    for r in ("bad_kf_front", "bad_kf_middle", "bad_kf_end"):
        sc2 = S.rule_scene(kind)
        sc2.kf_bad = []
        b2 = R.refresh(sc2, normals=False)[1]
        assert b2[at[r]] != best[at[r]], r                                              # ... and differs from the one with them counted
    assert st("all_kfs_bad") == R.DONE and chosen("all_kfs_bad") == -1 and not row_written("all_kfs_bad") and normal_written("all_kfs_bad")
    for r in ("point_bad", "point_unset"):
        assert st(r) == R.SKIPPED and chosen(r) == -1 and unchanged(sc.store[sc.rule[r]], store[sc.rule[r]], FIELDS)
    assert st("no_observations") == R.NO_OBSERVATIONS and unchanged(sc.store[sc.rule["no_observations"]], store[sc.rule["no_observations"]], FIELDS)
    for r in ("r1_ref_minus_one", "r1_ref_not_observing"):
        assert st(r) == R.NO_REF and not normal_written(r) and row_written(r) and chosen(r) >= 0
    for r in ("r2_zero_distance", "r2_not_finite"):
        assert st(r) == R.BAD_DISTANCE and not normal_written(r) and row_written(r)
    r = "ref_differs_from_chosen"
    e = best[at[r]]
    assert st(r) == R.DONE and sc.observations[e][1] != sc.ref_kf[sc.rule[r]]
    ref_obs = [o for o in sc.observations if o[0] == sc.rule[r] and o[1] == sc.ref_kf[sc.rule[r]]][0]
    assert store[sc.rule[r]]["ref_size"] == sc.size[ref_obs[1]][ref_obs[2]]             # the size of mpRefKF's observation, not the chosen row's
    if "pad_bytes_differ" in sc.rule:
        r = "pad_bytes_differ"
        rows = [sc.rows[o[1]][o[2]] for o in sc.observations if o[0] == sc.rule[r]]
        assert chosen(r) == 0 and R.distinctive(rows, False, 64)[0] == 1                # counted over the pitch, row 1 would win
    if "float_equal_distances" in sc.rule:
        r = "float_equal_distances"
        assert chosen(r) == 0 and med[at[r]] == np.float32(2.0)
    for pid in (100, 101, 102):
        assert unchanged(sc.store[pid], store[pid], FIELDS)


def test_restated_median_equals_a_sort():
    rng = np.random.RandomState(3)
    for n in (1, 2, 3, 4, 5, 8, 63, 64, 65):
        for _ in range(8):
            row = rng.randint(0, 12, n)
            assert R.median_of_row(row) == sorted(row)[int(0.5 * (n - 1))]
            frow = rng.rand(n).astype(np.float32)
            assert R.median_of_row(frow) == sorted(frow)[int(0.5 * (n - 1))]


def test_new_points_of_the_triangulation_are_a_fixed_point():
    """_tri_ref.new_point is UpdateNormalAndDepth for two observations (current, neighbour) with the current keyframe as mpRefKF"""
    import _tri_ref as T
    rng = np.random.RandomState(5)
    for _ in range(20):
        O1, O2, X = (rng.randn(3).astype(np.float32) for _ in range(3))
        X = X + np.float32(6)
        job = T.Job(np.eye(3), np.zeros(3), O1, np.eye(3), np.zeros(3), O2, max_size1=111.0, **{k: 1.0 for k in T.Job.FIELDS if k != "max_size1"})
        a = T.KF([0], [0], [np.float32(1.44)], [np.float32(37.2)])
        want = T.new_point(job, a, 0, X)
        st, got = R.normal_and_depth(X, [(0, 0), (1, 0)], [O1, O2], 0, lambda k, i: a.size[i], lambda k, i: a.sigma2[i], [job.max_size1, 1.0])
        assert st == R.DONE
        for k in R.PLANES:
            assert same(np.float32(want[k]), np.float32(got[k])), k


# ---- tools/refresh_host.cpp ----
def build_host(path):
    r = subprocess.run(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", str(path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fn = C.CDLL(str(path)).refresh_host
    fn.restype = None
    return fn


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("refresh_host") / "refresh_host.so")


def run_host(fn, sc, descriptors=True, normals=True):
    """tools/refresh_host.cpp on one scene -> (status, best_obs (an index into sc.observations), best_median, store {id: fields})"""
    op, ok, oi, order = S.edge_arrays(sc)
    npts = len(sc.point_ids)
    pt_ptr = np.zeros(npts + 1, np.int32)
    np.cumsum(np.bincount(op, minlength=npts), out=pt_ptr[1:])
    rows = np.stack([sc.rows[s] for s in range(sc.nslots)])
    sigma2, size = (np.stack([d[s] for s in range(sc.nslots)]).astype(np.float32) for d in (sc.sigma2, sc.size))
    ids = sorted(sc.store)
    capacity = max(ids) + 1
    st = {k: np.zeros((capacity,) + np.shape(sc.store[ids[0]][k]), np.asarray(sc.store[ids[0]][k]).dtype) for k in FIELDS if k != "descriptors"}
    st_rows = np.zeros((capacity, sc.pitch), np.uint8)
    for i in ids:
        for k in st:
            st[k][i] = sc.store[i][k]
        st_rows[i, :sc.desc_bytes] = np.ascontiguousarray(sc.store[i]["descriptors"]).view(np.uint8)
    where_k = {s: i for i, s in enumerate(sc.kfs)}
    slots, bad = np.array(sc.kfs, np.int32), np.array([s in sc.kf_bad for s in sc.kfs], np.uint8)
    centres, max_size = np.array([sc.centres[s] for s in sc.kfs], np.float32), np.array([sc.max_size[s] for s in sc.kfs], np.float32)
    pids, ref = np.array(sc.point_ids, np.int32), np.array([where_k.get(sc.ref_kf.get(p, -1), -1) for p in sc.point_ids], np.int32)
    status, best, med = (np.zeros(max(npts, 1), np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = lambda a: a if a.size else np.zeros(4, a.dtype)
    keep = [full(np.ascontiguousarray(a)) for a in (rows, sigma2, size, slots, centres, max_size, bad, pids, ref, pt_ptr, ok, oi)]
    fn(C.c_int(sc.cap), C.c_int(sc.pitch), C.c_int(sc.desc_bytes), C.c_int(sc.float_dim), p(keep[0]), p(keep[1]), p(keep[2]), C.c_int(len(slots)),
       p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]), C.c_int(npts), p(keep[7]), p(keep[8]), p(keep[9]), p(keep[10]), p(keep[11]),
       C.c_int(int(descriptors)), C.c_int(int(normals)), p(st["pos"]), p(st["normal"]), p(st["min_distance"]), p(st["max_distance"]), p(st["ref_size"]),
       p(st["ref_distance"]), p(st["ref_sigma"]), p(st["flags"]), p(st_rows), p(status), p(best), p(med))
    best = best[:npts]
    if len(order):
        best = np.where(best >= 0, order[np.maximum(best, 0)], -1).astype(np.int32)
    store = {}
    for i in ids:
        store[i] = {k: st[k][i] for k in st}
        raw = st_rows[i, :sc.desc_bytes]
        store[i]["descriptors"] = raw.view(np.float32).copy() if sc.float_dim else raw.copy()
    return status[:npts], best, (med[:npts].view(np.float32) if sc.float_dim else med[:npts]), store


def assert_same_answer(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("status", "best_obs", "best_median")):
        assert same(a, b), (what, name, a, b)
    assert sorted(got[3]) == sorted(want[3])
    for i in want[3]:
        for k in FIELDS:
            assert same(np.asarray(got[3][i][k], np.asarray(want[3][i][k]).dtype), want[3][i][k]), (what, i, k, got[3][i][k], want[3][i][k])


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
@pytest.mark.parametrize("parts", [(True, True), (True, False), (False, True)], ids=["both", "descriptors", "normals"])
def test_host_program_is_bit_equal_to_the_restatement_on_the_rules(host_program, kind, parts):
    sc = S.rule_scene(kind)
    want = rule_case(kind)[1] if parts == (True, True) else R.refresh(sc, *parts)
    assert_same_answer(run_host(host_program, sc, *parts), want, (kind, parts))


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_host_program_is_bit_equal_to_the_restatement_on_sized_points(host_program, kind):
    sc = S.sized_scene(kind, [1, 2, 3, 4, 0, 17, 33])
    assert_same_answer(run_host(host_program, sc), R.refresh(sc), kind)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "refresh_host"
    r = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DREFRESH_HOST_MAIN", SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "point 0 status 0 best_obs 0" in r.stdout and "point 1 status 0 best_obs 4" in r.stdout

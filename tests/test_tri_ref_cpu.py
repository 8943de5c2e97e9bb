"""CPU: the restatement of CreateNewMapPoints' match loop (tests/_tri_ref.py) on the scenes of tests/_tri_scenes.py - every constructed scene
ends in the status and route it is named after and its twin does not; the restated Jacobi returns the null vector numpy.linalg.svd finds in
float64; the composed neighbour loop gives a feature of the current keyframe at most one point."""
import numpy as np
import pytest

import _tri_ref as R
import _tri_scenes as S

# worst relative error of the restated x3D against numpy.linalg.svd in float64 on the same float32 matrix, over the noise-free seeded
# scenes below (4 kinds x 3 seeds x 48 matches), measured where this test was written: 8.13e-07.  Allowed: four times that.  Float against
# double error moves with the conditioning of A by a small factor; a Jacobi that returned another singular vector would miss by O(1).
SVD_WORST_MEASURED = 8.13e-07
SVD_BOUND = 4 * SVD_WORST_MEASURED


@pytest.mark.parametrize("name", sorted(S.EXPECT))
def test_constructed_scene_ends_where_it_is_named(name):
    s = S.scenes()[name]
    want = S.EXPECT[name]
    assert (s.status, s.route) == want, (name, R.STATUS_NAMES[s.status], s.route, s.on)
    assert (s.twin.status, s.twin.route) != want, (name, "the twin ends in the same place", s.on)


def test_every_status_and_route_is_reached():
    got = {(s.status, s.route) for s in S.all_constructed()}
    assert {st for st, _ in got} >= set(range(1, 11))
    assert {r for _, r in got} == {R.TRIANGULATED, R.UNPROJECT_A, R.UNPROJECT_B}


def test_parallax_scenes_sit_on_their_comparison():
    s = S.scenes()["cos_rays_zero"]
    assert not s.cos_rays() > 0 and s.twin.cos_rays() > 0
    s = S.scenes()["cos_rays_9998"]
    lo, hi = float(s.twin.cos_rays()), float(s.cos_rays())
    assert lo < 0.9998 <= hi
    f = np.float32(0.9998)                                      # the float above the double literal; its neighbour below is the float under it
    assert s.cos_rays() == f and s.twin.cos_rays() == np.nextafter(f, np.float32(0))


def test_reprojection_scenes_sit_between_two_floats_of_sigma2():
    for name, key, f in (("reproj1_mono", "fa", 5.991), ("reproj2_mono", "fb", 5.991), ("reproj1_stereo", "fa", 7.8), ("reproj2_stereo", "fb", 7.8)):
        s = S.scenes()[name]
        a, b = getattr(s, key)["sigma2"], getattr(s.twin, key)["sigma2"]
        assert np.nextafter(a, np.float32(np.inf)) == b, name      # the gate rejects at sigma2 and accepts one ulp above
        assert s.twin.status == R.ACCEPTED, name


def test_random_scenes_reach_the_stereo_routes():
    routes, statuses = set(), set()
    for kind in S.KINDS:
        for seed in S.SEEDS:
            job, a, b, m = S.random_scene(kind, seed)
            st, rt, _, new_id, n_new, pts = R.triangulate([job], [a], [b], m[None, :])
            routes |= set(rt[0][st[0] == R.ACCEPTED].tolist())
            statuses |= set(st[0].tolist())
            assert n_new[0] == len(pts) == int((new_id >= 0).sum())
            assert [p[0] for p in pts] == list(range(len(pts)))          # dense ids in ascending feature order
    assert routes == {0, 1, 2} and {R.ACCEPTED, R.LOW_PARALLAX, R.REPROJ1, R.REPROJ2, R.SCALE_RATIO, R.NO_MATCH} <= statuses


def test_restated_jacobi_finds_the_null_vector_numpy_finds():
    worst = 0.0
    for kind in S.KINDS:
        for seed in S.SEEDS:
            job, a, b, m = S.random_scene(kind, seed, clean=True)
            for i in range(a.n):
                xn1, xn2, _, _ = R._rays(job, a, i, b, int(m[i]))
                A = R.triangulation_matrix(job, xn1, xn2)
                v, sweeps = R.jacobi_null_vector(A)
                assert sweeps < R.JACOBI_SWEEPS
                x = (v[:3] / v[3]).astype(np.float64)
                vt = np.linalg.svd(A.astype(np.float64))[2][3]
                y = vt[:3] / vt[3]
                worst = max(worst, float(np.linalg.norm(x - y) / np.linalg.norm(y)))
    print("worst relative error %.3e, measured when written %.3e, bound %.3e" % (worst, SVD_WORST_MEASURED, SVD_BOUND))
    assert worst <= SVD_BOUND


def test_new_point_fields():
    s = S.scenes()["ratio_low"].twin
    assert s.status == R.ACCEPTED
    a = S.kf_of([s.fa])
    f = R.new_point(s.job, a, 0, s.x3d)
    assert np.array_equal(f["pos"], s.x3d) and f["flags"] == 5
    assert abs(float(np.linalg.norm(f["normal"])) - 1.0) < 1e-2     # two nearly parallel unit vectors, halved
    assert f["max_distance"] == f["ref_distance"] * a.size[0] and f["min_distance"] == f["max_distance"] / s.job.max_size1
    assert f["ref_sigma"] == np.sqrt(a.sigma2[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_composed_loop_gives_a_feature_at_most_one_point(seed):
    W = S.World(seed)
    none = lambda: [np.zeros(W.n, np.uint8) for _ in range(W.nn)]
    pts = R.create_new_map_points(W.kfs[0], W.kfs[1:], W.jobs, W.search(60.0), np.zeros(W.n, np.uint8), none())
    feats = [i for _, _, i, _, _ in pts]
    assert len(feats) > W.n // 2 and len(set(feats)) == len(feats)
    assert [p[0] for p in pts] == list(range(len(pts)))
    assert len({k for _, k, _, _, _ in pts}) > 1 or len(feats) == W.n      # later neighbours pick up what the first left
    # the same neighbours with masks that never move (one batched call) create a point per neighbour for the same feature
    stale = []
    for k in range(W.nn):
        m = W.search(60.0)(k, np.zeros(W.n, np.uint8), np.zeros(W.n, np.uint8))
        stale += [i for i in range(W.n) if R.triangulate_match(W.jobs[k], W.kfs[0], i, W.kfs[k + 1], int(m[i]))[0] == R.ACCEPTED]
    assert len(set(stale)) < len(stale)

"""CPU: the oracle's projection searches against the plain-Python restatement of the reference (tests/_proj_ref.py) on the constructed scenes of
tests/_proj_scenes.py, and the proof that every scene reaches the branch it exists for: the equality counter of its rule is > 0 AND the
restatement with that one comparison flipped gives another answer.  Without these checks tests/test_gpu_proj_scenes.py could stay green
without testing anything.

The constants of the kernels the scenes are built to exceed (nothing is imported from the kernels):
  PK = 4         csrc/k_project.hip:37   keys per query of the projection searches
  IK = 8         csrc/k_project.hip:38   keys per query of SearchForInitialization
  PW_LIST = 256  csrc/k_project.hip:178  slots of the dense candidate list; a chunk is 64 lanes x PW_CPL = 4 cells = 256 cells (:128)
  PW_T = 1024    csrc/k_project.hip:675  threads of the fixed point: live queries are taken 1024 at a time (`tid < nlive`)
  the fixed point runs when its tables fit 150 KiB - 32 KiB - 2 KiB of LDS (afv_project_prepare in k_project.hip, choose_route in afv_project.hip);
  the ordered walk stages the queries' records in LDS while 33920 + 64 * nq <= 128 KiB (k_project.hip:421-422, :1731-1732).
"""
import numpy as np
import pytest

import _proj_ref as R
import _proj_scenes as PS

PK, IK, PW_LIST, PW_T = 4, 8, 256, 1024
WG_LDS_MAX, WALK_FIXED, WALK_REC, WALK_MAX = R.WG_LDS_MAX, R.WALK_FIXED, R.WALK_REC, R.WALK_MAX
proj_wg_lds, init_wg_lds = R.proj_wg_lds, R.init_wg_lds
# a size-regime scene goes through the Python loops only below this many candidate visits (the two largest go to the oracle alone).  The
# constructed scenes - 274 cases, each run plain and flipped - are what the file's time is made of; DESIGN_LOG.md has the figures
MAX_VISITS = 100000

CASES = PS.all_constructed()


def run_oracle(oracle, c):
    if c.kind == "init":
        return oracle.match_initialization(c.F, c.Q, **c.kw)
    return oracle.match_projection(c.F, c.Q, **c.kw)


_REF = {}


def run_ref(c, flip=None):
    """(the unflipped answers are kept: several tests read the same traces)"""
    if flip is None and c.name in _REF:
        return _REF[c.name]
    if c.kind == "init":
        r = R.match_initialization(c.F, c.Q, flip=flip, **c.kw)
    else:
        r = R.match_projection(c.F, c.Q, flip=flip, **c.kw)
    if flip is None:
        _REF[c.name] = r
    return r


def test_scene_names_are_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_oracle_equals_restatement_and_the_scene_reaches_its_rule(oracle, c):
    want, wn = run_oracle(oracle, c)
    got, n, tr = run_ref(c)
    assert n == wn and np.array_equal(got, want)
    if c.rule is None:
        return
    if c.rule != "steal_hist_stays":
        assert tr["eq"][c.rule] > 0, "the scene never meets its rule at equality"
    else:
        assert tr["steals"] >= 30
    if c.rule == "pos_round":
        assert tr["half_cells"] >= 3   # both axes inside the grid and at least one left of / above it
    if c.rule.startswith("skip_"):
        assert tr["skip"][c.rule[5:]] == 1 and sum(tr["clip"].values()) >= 1
    flipped, fn, _ = run_ref(c, flip=c.rule)
    assert not np.array_equal(flipped, got), "the outcome does not depend on the rule: the scene proves nothing"


def _by(prefix, suffix):
    """the cases of one generator and search kind, every descriptor kind and grid"""
    return [c for c in CASES if c.name.split("-b")[0].split("-f")[0] == prefix and ("-" + suffix) in c.name]


@pytest.mark.parametrize("suffix,K", [("localmap", PK), ("lastframe", PK), ("init", IK)])
def test_ordered_phase_stress_scenes(suffix, K):
    for c in _by("chain", suffix):
        got, n, tr = run_ref(c)
        assert tr["longest_chain"] >= 256, (c.name, tr["longest_chain"])
        assert n == c.Q.n
    for c in _by("behind", suffix):
        got, n, tr = run_ref(c)
        assert int((tr["rank"] >= K).sum()) >= 32 and int((tr["rank"] >= 64).sum()) >= 8, c.name
        assert tr["starved"] >= 1 and int(tr["ncand"].max()) > K
        if suffix != "init":
            assert tr["drop"]["occupied"] > 0
    if suffix != "init":
        for c in _by("chain-nonocc", suffix) + _by("behind-nonocc", suffix):
            got, n, tr = run_ref(c)
            assert c.Q.occupies is not None and 0 < int(c.Q.occupies.sum()) < c.Q.n
            assert n > int((got >= 0).sum())  # some feature was taken twice: a query that does not occupy was overwritten
            assert tr["longest_chain"] >= (PK if c.name.startswith("chain") else 1)


def test_trace_counters_on_the_filter_scenes():
    tot = {}
    for c in CASES:
        if "b32" in c.name and c.name.split("-")[0] in ("dx_lt_r", "size_lt_min", "size_gt_max", "dy_lt_r", "uright_ge0", "er_gt_max", "mdist_le"):
            tr = run_ref(c)[2]
            for k, v in tr["drop"].items():
                tot[k] = tot.get(k, 0) + v
    for k in ("size_low", "size_high", "dx", "dy", "stereo", "chi2_3dof", "mdist"):
        assert tot[k] > 0, k


def test_generators_are_deterministic():
    again = PS.all_constructed()
    assert len(again) == len(CASES)
    for a, b in zip(CASES, again):
        assert a.name == b.name and a.kw == b.kw
        for o1, o2 in ((a.F, b.F), (a.Q, b.Q)):
            for k, v in o1.__dict__.items():
                w = o2.__dict__[k]
                assert (v is None and w is None) or np.array_equal(np.asarray(v), np.asarray(w)), (a.name, k)
    s1, s2 = PS.size_regimes(), PS.size_regimes()
    for k in s1:
        for o1, o2 in zip(s1[k], s2[k]):
            for a, v in o1.__dict__.items():
                assert (v is None and o2.__dict__[a] is None) or np.array_equal(np.asarray(v), np.asarray(o2.__dict__[a])), (k, a)


@pytest.mark.parametrize("seed,shift,rs", [(1, 4, 15.0), (2, 7, 12.0), (5, 5, 15.0), (21, 5, 10.0)])
def test_random_scenes_from_the_oracles_extractor(oracle, seed, shift, rs):
    F, Q = PS.random_scene(oracle, seed, shift, rs)
    for kw in (dict(th_high=75.0, nnratio=0.8), dict(th_high=75.0, nnratio=0.9, check_orientation=True, last_frame=True), dict(th_high=75.0, fuse=True)):
        want, wn = oracle.match_projection(F, Q, **kw)
        got, n, tr = R.match_projection(F, Q, **kw)
        assert n == wn and np.array_equal(got, want) and wn > 100, kw
    want, wn = oracle.match_initialization(F, Q, th_low=75.0, nnratio=0.9, check_orientation=True)
    got, n, tr = R.match_initialization(F, Q, th_low=75.0, nnratio=0.9, check_orientation=True)
    assert n == wn and np.array_equal(got, want) and wn > 100


def test_sim3_agreement(oracle):
    """SearchBySim3 on a random scene: KF1's features are the scene's queries (placed where they project), KF2's the scene's features"""
    F, Q = PS.random_scene(oracle, 3, 3, 10.0)
    m = min(Q.n, F.N)   # SearchBySim3 wants nq of one side == n of the other
    afv = PS.afv
    F2 = afv.FrameGridView(F.descriptors[:m], np.stack([F.x[:m], F.y[:m]], 1), F.sizes[:m])
    Q1 = afv.ProjectionQueries(Q.descriptors[:m], Q.u[:m], Q.v[:m], Q.r[:m], Q.min_size[:m], Q.max_size[:m])
    F1 = afv.FrameGridView(Q1.descriptors, np.stack([Q1.u, Q1.v], 1), (Q1.min_size * np.float32(1.2)))
    Q2 = afv.ProjectionQueries(F2.descriptors, F2.x, F2.y, np.full(m, 12.0, np.float32), F2.sizes / np.float32(1.3), F2.sizes * np.float32(1.3))
    want, wn = oracle.match_sim3(F2, Q1, F1, Q2, th_high=75.0)
    got, n, _ = R.match_sim3(F2, Q1, F1, Q2, th_high=75.0)
    assert n == wn and np.array_equal(got, want) and wn > 50


# ---- size regimes: which side of which limit every scene lies on ----
REGIMES = PS.size_regimes()


def test_size_regimes_lie_on_both_sides_of_the_limits():
    side = {k: (proj_wg_lds(F.N, Q.n) <= WG_LDS_MAX, WALK_FIXED + WALK_REC * Q.n <= WALK_MAX) for k, (F, Q) in REGIMES.items()}
    # (fixed point runs, ordered walk stages its records)
    assert side["n8192-nq1"] == (True, True)
    assert side["n8192-nq1500"] == (False, True)      # 98304 + 1536 * 33 + 64 = 149056 > 118784; 33920 + 64 * 1500 = 129920 <= 131072
    assert side["n8192-nq9000"] == (False, False)
    assert side["n8192-nq65535"] == (False, False)
    assert side["live2500-rescans"] == (True, False)
    # the two walk regimes with the fixed point out of reach: staged below 1520 queries, unstaged above
    assert WALK_FIXED + WALK_REC * 1500 <= WALK_MAX < WALK_FIXED + WALK_REC * 2500
    # SearchForInitialization on the same scenes (tests/test_gpu_proj_scenes.py sends every regime through it): its fixed point runs on the
    # small ones only, and never above 32767 queries (16-bit tables, choose_route in afv_project.hip)
    iside = {k: init_wg_lds(F.N, Q.n) <= WG_LDS_MAX and Q.n <= 32767 for k, (F, Q) in REGIMES.items()}
    assert iside["grid-1x1"] and iside["chunk-256"] and iside["n3000-cluster-64x48"]
    assert not iside["live2500-rescans"] and not iside["n8192-nq1"] and not iside["grid-8192-cells"]
    assert REGIMES["n8192-nq65535"][1].n > 32767 >= REGIMES["n8192-nq9000"][1].n
    assert side["grid-8192-cells"] == (True, True) and side["n3000-cluster-64x48"] == (True, True)


def test_the_library_agrees_with_the_restated_lds_formulas(afv):
    """afv_project_wg_lds is a host function of the built library"""
    import ctypes as C
    lib = C.CDLL(afv._lib.LIB_PATH)   # loads without a device; a library that does not load is a failure, not a skip
    lib.afv_project_wg_lds.restype = C.c_size_t
    lib.afv_project_wg_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    for n, nq in [(0, 0), (1, 1), (1000, 1000), (8192, 1), (8192, 1500), (8192, 9000), (8192, 65535), (400, 2500), (63, 65), (64, 64)]:
        assert lib.afv_project_wg_lds(0, n, nq, 0) == proj_wg_lds(n, nq)
        assert lib.afv_project_wg_lds(0, n, nq, 1) == proj_wg_lds(n, nq, True)
        assert lib.afv_project_wg_lds(1, n, nq, 0) == init_wg_lds(n, nq)


@pytest.mark.parametrize("name", list(REGIMES))
def test_size_regime_scenes(oracle, name):
    F, Q = REGIMES[name]
    kws = [dict(th_high=75.0, nnratio=0.8), dict(th_high=75.0, nnratio=0.9, check_orientation=True, last_frame=True)]
    visits = R.candidate_visits(F, Q)
    for kw in kws:
        want, wn = oracle.match_projection(F, Q, **kw)
        assert len(want) == F.N
        if Q.n >= 300:
            assert wn > 20, (name, kw, wn)
        if visits <= MAX_VISITS:
            got, n, tr = R.match_projection(F, Q, **kw)
            assert n == wn and np.array_equal(got, want)
            if name.startswith("n3000-cluster"):
                assert tr["chunk_max"] > PW_LIST
            if name == "chunk-256":   # `total_ <= PW_LIST` at equality: the dense list exactly full ...
                assert tr["chunk_counts"] - {0} == {PW_LIST}
            if name == "chunk-257":   # ... and the first count that takes the per-lane fallback
                assert tr["chunk_counts"] - {0} == {PW_LIST + 1}
            if name == "live2500-rescans" and kw.get("last_frame"):
                # live as the kernel lists it (a key that was free before the call, within the threshold); a query needs the rescan when its
                # answer lies behind the PK keys drawn from exactly those candidates
                live = np.nonzero(tr["live"])[0]
                deep = live[tr["key_rank"][live] >= PK]
                pos = np.searchsorted(live, deep)   # position among the live queries
                print("live %d, answers behind the key list %d, of them at live position >= 1024: %d, >= 2048: %d"
                      % (len(live), len(deep), int((pos >= PW_T).sum()), int((pos >= 2 * PW_T).sum())))
                assert len(live) > 2 * PW_T and (pos >= PW_T).any() and (pos >= 2 * PW_T).any()
    if name.startswith(("n3000-cluster", "chunk-")) or name == "live2500-rescans":
        assert visits <= MAX_VISITS, "this scene's branch reach is proved by the restatement's trace"


@pytest.mark.parametrize("desc", ["b32", "f64"])
def test_the_every_route_scene_needs_its_masks_its_histogram_and_its_order(oracle, desc):
    """PS.every_route_scene (tests/test_gpu_proj_scenes.py::test_one_scene_through_every_projection_route): the oracle equals the
    restatement on every search the GPU test sends it through; a third of the queries match; a query's first choice is held by an earlier
    query of the same call, and SearchForInitialization sees features change hands; the answer changes when the occupancy mask, the holes
    in qvalid, the orientation check, the stereo gate or the chi-square gate is taken away - so a route that drops one of them shows"""
    import copy
    s = PS.every_route_scene(desc)
    F, Q = s["F"], s["Q"]
    assert F.N == 70 and Q.n == 65 and 0 < int(F.occupied.sum()) < 8 and 0 < int((Q.valid == 0).sum()) < 8 and Q.valid[64]
    kw = dict(th_high=75.0, nnratio=0.9, check_orientation=True, last_frame=True)
    got, n, tr = R.match_projection(F, Q, **kw)
    want, wn = oracle.match_projection(F, Q, **kw)
    assert n == wn and np.array_equal(got, want)
    assert 3 * n >= Q.n
    assert tr["longest_chain"] >= 1 and tr["drop"]["occupied"] > 0
    bare = copy.copy(F); bare.occupied = None
    assert not np.array_equal(oracle.match_projection(bare, Q, **kw)[0], want)
    allq = copy.copy(Q); allq.valid = None
    assert not np.array_equal(oracle.match_projection(F, allq, **kw)[0], want)
    assert oracle.match_projection(F, Q, **dict(kw, check_orientation=False))[1] > n
    gs, ns, trs = R.match_projection(s["Fs"], s["Qs"], **kw)
    ws, wsn = oracle.match_projection(s["Fs"], s["Qs"], **kw)
    assert ns == wsn and np.array_equal(gs, ws) and trs["drop"]["stereo"] > 0 and not np.array_equal(ws, want) and 3 * ns >= Q.n
    fkw = dict(th_high=75.0, fuse=True)
    for Fx, Qx in ((F, Q), (s["F1"], s["Q2"])):
        g, gn, _ = R.match_projection(Fx, Qx, **fkw)
        w, wn2 = oracle.match_projection(Fx, Qx, **fkw)
        assert gn == wn2 and np.array_equal(g, w) and 3 * gn >= Qx.n
    Fi = copy.copy(F); Fi.inf = (np.float32(1.0) / (F.sizes * F.sizes)).astype(np.float32)
    g, gn, trf = R.match_projection(Fi, Q, **fkw)
    w, wn2 = oracle.match_projection(Fi, Q, **fkw)
    assert gn == wn2 and np.array_equal(g, w) and trf["drop"]["chi2_2dof"] > 0 and gn < oracle.match_projection(F, Q, **fkw)[1]
    g, gn, _ = R.match_sim3(F, Q, s["F1"], s["Q2"], th_high=75.0)
    w, wn2 = oracle.match_sim3(F, Q, s["F1"], s["Q2"], th_high=75.0)
    assert gn == wn2 and np.array_equal(g, w) and 3 * gn >= Q.n
    ikw = dict(th_low=75.0, nnratio=0.9, check_orientation=True)
    for Qx in (s["Qi"], Q):
        g, gn, tri = R.match_initialization(F, Qx, **ikw)
        w, wn2 = oracle.match_initialization(F, Qx, **ikw)
        assert gn == wn2 and np.array_equal(g, w) and 3 * gn >= Q.n and tri["steals"] >= 1
    assert float(F.sizes.max()) < PS.INIT_MAX_SIZE and bool(np.all(Q.r == Q.r[0]))   # what the call between resident frames can state

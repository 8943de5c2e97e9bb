"""-m gpu: the constructed scenes of tests/_pairs_scenes.py through every route to k_match_topk, k_match_topk_mfma (8 and 16 dwords per row,
sliced and unsliced), k_match_resolve and k_match_resolve_wg.  tests/test_pairs_ref_cpu.py proves on the CPU that every scene reaches the
branch it is named for and that the record models satisfy the contract.

A ROUTE is (phase-1 engine, phase-2 engine, small-batch mode, call size) for a row width:
  phase-1 engine     0 popcount, 1 matrix cores
  phase-2 engine     0 the walk on one wavefront, 1 the workgroup-wide fixed point
  small-batch mode   0 never; 2 always = column slices, with engine 1 only (afv_match_topk_slices gives the popcount engine one slice)
  call size          "chunks" of at most 8 pairs (rescans through L2); "all" pairs of a ratio group in one call, padded with repeats to at
                     least 9 (columns staged in LDS where cap <= 1024, or 512 for 64-byte rows)
  row width          b32: 8 dwords through FeatureMatcher.match_pairs_device; b61: 16 dwords through a 61-byte DescriptorTable
Every scene takes every route (CANNOT is empty and says so); a call takes one ratio, so a route is one call per ratio group.

Per call, after torch.cuda.synchronize(): match[p, :n1], the -1 fill behind n1 and nmatches equal the oracle's; the records read from
d_topk satisfy record_contract and equal the record model slot for slot and nk; on the sliced routes every slice's record (d_slice)
satisfies the contract over its own columns and equals the model's; the first call of a route makes the buffers exist, the scratch is
painted 0xA5 and the call repeated: what is checked is the second call, and the record rows >= n1 of every pair are still painted.
Everything is an integer and compared for equality.  Failures are collected over all scenes and reported together.
"""
import numpy as np
import pytest

import _pairs_ref as P
import _pairs_scenes as PS

pytestmark = pytest.mark.gpu

ENGINES = [(e1, e2, mode) for e1 in (0, 1) for e2 in (0, 1) for mode in (0, 2) if not (mode == 2 and e1 == 0)]
ENGINE_IDS = ["%s-%s-%s" % (("popcount", "mfma")[e1], ("walk", "wg")[e2], ("unsliced", "sliced")[mode // 2]) for e1, e2, mode in ENGINES]
SIZES = ("chunks", "all")
# scenes that cannot take a route, with the reason: none - every scene is a pair of valid descriptor sets within cap, and every route takes those
CANNOT = {(eng, size): {} for eng in ENGINES for size in SIZES}
PAINT = 0xA5
_SCENES, _MODEL, _WANT, _CONTRACT = {}, {}, {}, {}


def scenes_of(kind, which):
    if (kind, which) not in _SCENES:
        _SCENES[kind, which] = PS.small_scenes(kind) if which == "small" else {"cap1300": [PS.live_behind_1024(kind)], "cap4096": [PS.largest_capacity(kind)]}[which]
    return _SCENES[kind, which]


def model_of(s, name):
    """the distances, the three record models and the per-slice records of a scene: computed once, never changed"""
    if s.name not in _MODEL:
        dist = P.hamming(s.D1, s.D2)
        nsl = P.topk_slices(s.cap, 1)
        merged, per = P.records_sliced(dist, nsl)
        _MODEL[s.name] = dict(dist=dist, popcount=P.records_popcount(dist), mfma=P.records_mfma(dist), sliced=merged, per=per,
                              cols=P.slice_columns(dist.shape[1], nsl), nslices=nsl)
    return _MODEL[s.name][name]


def want_of(oracle, s):
    if s.name not in _WANT:
        _WANT[s.name] = oracle.search_by_bow_kf_kf(s.D1, s.D2, angle1=s.a1, angle2=s.a2, th_low=PS.TH[s.kind], nnratio=s.ratio, check_orientation=s.ori)
    return _WANT[s.name]


def contract_of(s, recs, tag):
    """record_contract over all rows of a scene; the verdict is kept per distinct record array (most routes write the same records)"""
    k = (s.name, tag, recs.tobytes())
    if k not in _CONTRACT:
        dist = model_of(s, "dist")
        n2 = dist.shape[1]
        if tag == "merged":
            bad = [(i, msg) for i in range(len(recs)) for msg in [P.record_contract(recs[i], dist[i], n2)] if msg]
        else:
            cols = model_of(s, "cols")
            bad = [(i, q, msg) for i in range(len(recs)) for q in range(recs.shape[1])
                   for msg in [P.record_contract(recs[i, q], dist[i, cols[q]], len(cols[q]), cols[q])] if msg]
        _CONTRACT[k] = bad[:3]
    return _CONTRACT[k]


@pytest.fixture(scope="module")
def ctx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context()
    yield c
    c.close()


class Runner:
    """the scenes of one kind and capacity, resident: b32 as torch tensors for match_pairs_device, b61 as a DescriptorTable"""

    def __init__(self, afv, ctx, kind, scenes):
        import torch
        self.afv, self.ctx, self.kind, self.scenes, self.torch = afv, ctx, kind, scenes, torch
        self.cap = scenes[0].cap
        t, a, n = PS.table_of(scenes)
        self.table = None
        if kind == "b32":
            kps = np.zeros((len(t), self.cap), afv.KP_DTYPE)
            kps["angle"] = a
            self.desc = torch.from_numpy(t).cuda()
            self.kps = torch.from_numpy(kps.view(np.float32).reshape(len(t), self.cap, 7)).cuda()
            self.n = torch.from_numpy(n).cuda()
            self.matcher = afv.FeatureMatcher(0.6, True, ctx=ctx)
        else:
            self.table = afv.table.DescriptorTable(ctx, len(t), self.cap, desc_bytes=PS.nbytes(kind))
            assert self.table.pitch == 64
            for k in range(len(t)):
                self.table.set(k, t[k, :n[k]], a[k, :n[k]])

    def close(self):
        if self.table is not None:
            self.table.close()

    def call(self, idx, ratio, ori):
        torch = self.torch
        pa = torch.tensor([2 * i for i in idx], dtype=torch.int32, device="cuda")
        pb = torch.tensor([2 * i + 1 for i in idx], dtype=torch.int32, device="cuda")
        th = PS.TH[self.kind]
        if self.table is None:
            self.matcher.mfNNratio = float(ratio)
            m, nm = self.matcher.match_pairs_device(self.desc, self.kps, self.n, pa, pb, th_low=th, check_orientation=ori)
        else:
            m, nm = self.table.match_pairs_device(pa, pb, th, ratio, ori)
        torch.cuda.synchronize()
        return m.cpu().numpy(), nm.cpu().numpy()

    def route(self, oracle, eng, size):
        """every call of the route: first call, paint, second call, checks.  Returns (failures, names of the scenes that ran)"""
        e1, e2, mode = eng
        ctx, cap = self.ctx, self.cap
        sliced = mode == 2
        nsl = P.topk_slices(cap, e1) if sliced else 1
        assert ctx.lib.afv_match_topk_slices(cap, e1, ((cap + 63) // 64 + 1) // 2) == P.topk_slices(cap, e1)
        model = "popcount" if e1 == 0 else ("sliced" if sliced else "mfma")
        bad, ran = [], set()
        for ratio, ori, idx in PS.calls_of(self.scenes, size):
            assert (len(idx) <= 8) if size == "chunks" else (len(idx) >= 9)
            self.call(idx, ratio, ori)
            ctx.paint_scratch(PAINT)
            m, nm = self.call(idx, ratio, ori)
            topk = ctx.scratch_read("d_topk", 0, len(idx) * cap * 32).view(np.int32).reshape(len(idx), cap, 8)
            per = ctx.scratch_read("d_slice", 0, len(idx) * cap * nsl * 32).view(np.int32).reshape(len(idx), cap, nsl, 8) if sliced else None
            for p, i in enumerate(idx):
                s = self.scenes[i]
                ran.add(s.name)
                n1 = len(s.D1)
                want, wn = want_of(oracle, s)
                tag = "%s[pair %d]" % (s.name, p)
                if int(nm[p]) != wn or not np.array_equal(m[p, :n1], want):
                    rows = np.nonzero(m[p, :n1] != want)[0][:4].tolist()
                    bad.append("%s: outputs differ (count %d, oracle %d; rows %s)" % (tag, nm[p], wn, rows))
                if not np.all(m[p, n1:] == -1):
                    bad.append("%s: match behind n1 is not -1" % tag)
                recs = np.ascontiguousarray(topk[p, :n1])
                c = contract_of(s, recs, "merged")
                if c:
                    bad.append("%s: record contract %s" % (tag, c))
                if not np.array_equal(recs, model_of(s, model)):
                    rows = np.nonzero((recs != model_of(s, model)).any(1))[0][:4].tolist()
                    bad.append("%s: records != %s model at rows %s (first: %s, model %s)" % (tag, model, rows, recs[rows[0]].tolist(), model_of(s, model)[rows[0]].tolist()))
                if not np.all(topk[p, n1:].view(np.uint8) == PAINT):
                    bad.append("%s: record rows >= n1 were written" % tag)
                if sliced:
                    assert nsl == model_of(s, "nslices")
                    sl = np.ascontiguousarray(per[p, :n1])
                    c = contract_of(s, sl, "slices")
                    if c:
                        bad.append("%s: slice record contract %s" % (tag, c))
                    if not np.array_equal(sl, model_of(s, "per")):
                        bad.append("%s: slice records != model" % tag)
        return bad, ran


def run_routes(afv, oracle, ctx, kind, which, engines):
    scenes = scenes_of(kind, which)
    r = Runner(afv, ctx, kind, scenes)
    bad = []
    try:
        for eng in engines:
            ctx.set_match_engine(eng[0])
            ctx.set_match_resolve(eng[1])
            ctx.set_small_batch_path(eng[2])
            for size in SIZES:
                b, ran = r.route(oracle, eng, size)
                left_out = {s.name for s in scenes} - ran
                assert left_out == set(CANNOT[eng, size]), left_out
                bad += ["[%s %s] %s" % (ENGINE_IDS[ENGINES.index(eng)], size, x) for x in b]
    finally:
        ctx.set_match_engine(1)       # the context's defaults (afv_create), as tests/test_gpu_table_widths.py restores them
        ctx.set_match_resolve(2)
        ctx.set_small_batch_path(1, 4)
        r.close()
    return bad


@pytest.mark.parametrize("kind", PS.KINDS)
@pytest.mark.parametrize("eng", ENGINES, ids=ENGINE_IDS)
def test_cap320_scenes_on_every_route(afv, oracle, ctx, eng, kind):
    """all scenes of cap 320, both call sizes"""
    bad = run_routes(afv, oracle, ctx, kind, "small", [eng])
    assert bad == [], "\n".join(bad)


@pytest.mark.parametrize("kind", PS.KINDS)
@pytest.mark.parametrize("which", ["cap1300", "cap4096"])
def test_large_scenes_on_every_route(afv, oracle, ctx, which, kind):
    """the two large scenes in calls of their own: about 1090 live rows with the contention behind live slot 1024 (cap 1300: records read
    from global memory, the one-at-a-time path of the workgroup form, eleven slices), and cap 4096, the largest the entry point accepts
    (it is accepted and the workgroup form's LDS fits: nothing had to be lowered)"""
    bad = run_routes(afv, oracle, ctx, kind, which, ENGINES)
    assert bad == [], "\n".join(bad)

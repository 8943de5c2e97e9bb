"""-m gpu: every device entry point that stages through a context must not depend on what an earlier call left in the context's grow-only
scratch (d_match, its pinned image h_stage, d_topk, d_slice, d_l2_scratch, the staging of stores and tables), and must leave the
zero-at-rest words (d_proj_ticket, d_points_count, d_tickets) zero.  The session's shared context cannot show either: what is left in its
buffers is usually the same entry point's own data at the same offsets.

Every row of tests/_scratch_cases.py runs on a context of its own: first call (the buffers grow inside it), then again after
afv_debug_paint_scratch(0x00) and after (0xFF) - as floats and doubles NaN, as ints -1, every flag byte set - with the answers held to the
module's own expected bytes each time, the buffer sizes unchanged between the passes, and the rest words read after every call.  The
role chains run different layouts over the same bytes, alone, chained and chained with a repaint between the steps, and three roles run
at once on three threads.  test_painting_reaches_the_buffers shows that the paint lands where the calls stage."""
import os
import threading
import time

import numpy as np
import pytest

import _scratch_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture
def fresh(afv):
    """contexts made for one test and closed with it"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = []

    def make(**kw):
        made.append(afv.Context(**dict(SC.CTX, **kw)))
        return made[-1]
    yield make
    for c in made:
        c.close()


SLOT = {name: i for i, name in enumerate(("d_match", "h_stage", "d_topk", "d_slice", "d_l2_scratch", "points_stage", "points_pin", "table_pairs", "table_pin"))}


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_entry_point_on_painted_scratch(afv, oracle, fresh, case):
    lib = afv._lib.load()
    with SC.recording(lib, afv._lib.SYMBOLS) as called:
        ctx = fresh(**case.ctx)
        step = case.make(afv, ctx, oracle)
        try:
            sizes = None
            for what, byte in (("first call on a fresh context", None), ("scratch painted 0x00", 0x00), ("scratch painted 0xFF", 0xFF)):
                if byte is not None:
                    sizes = ctx.scratch_bytes()
                    if "points" in case.holds:       # the row's store is alive: its staging is there to be painted
                        assert sizes[SLOT["points_stage"]] > 0 and sizes[SLOT["points_pin"]] > 0, (case.name, what, sizes)
                    if "tables" in case.holds:
                        assert sizes[SLOT["table_pairs"]] > 0 and sizes[SLOT["table_pin"]] > 0, (case.name, what, sizes)
                    ctx.paint_scratch(byte)
                called.clear()
                step()                                   # the answer against the module's expected bytes
                missing = [e for e in case.entries if e not in called]
                assert not missing, (case.name, what, "the step never called", missing)
                assert ctx.rest_words() == 0, (case.name, what, "a zero-at-rest word is not zero")
                if byte is not None:                     # the call ran entirely inside painted memory
                    assert ctx.scratch_bytes() == sizes, (case.name, what, dict(zip(ctx.SCRATCH_NAMES, zip(sizes, ctx.scratch_bytes()))))
        finally:
            if hasattr(step, "close"):
                step.close()
        called.clear()
        ctx.close()
        assert "afv_destroy" in called


def test_painting_reaches_the_buffers(afv, oracle, fresh):
    """the control: after a paint every painted buffer reads back as the byte - head and tail of the context's five, every byte of the
    staging of the store and of the pair buffers of the two tables; after one afv_frame_pose_optimize the head of d_match is the staged
    pts array"""
    ctx = fresh()
    assert tuple(ctx.SCRATCH_NAMES) == tuple(SLOT)
    # grow every buffer: a pose optimisation (store), a float pair match, pair calls on a small table and, for the column slices, one
    # pair of two keyframes of 1000 rows (a call of at most four pairs over wide sets is dealt to slices)
    s, rig = SC.pose_rig(afv, ctx)
    table = wide = None
    try:
        rig.frame.PoseOptimizationBatch(rig.points, [s.pts])
        SC.reuse("test_gpu_match", "test_l2_pairs_in_several_launches_with_a_ragged_last_one")(afv, ctx, oracle)()
        table, host, _, _ = SC.small_table(afv, ctx)
        table.match_pairs([0, 1], [1, 2], 75.0, 0.6)
        rows, angles, counts = afv.synth.keyframe_table(2, 1000)
        wide = afv.table.DescriptorTable(ctx, 2, 1000)
        for k in range(2):
            wide.set(k, rows[k, :counts[k]], angles[k, :counts[k]])
        m, nm = wide.match_pairs([0], [1], 75.0, 0.6)
        want, wn = oracle.search_by_bow_kf_kf(rows[0, :counts[0]], rows[1, :counts[1]], angle1=angles[0, :counts[0]], angle2=angles[1, :counts[1]],
                                              th_low=75.0, nnratio=0.6, check_orientation=True)
        assert nm[0] == wn and np.array_equal(m[0, :counts[0]], want)
        sizes = ctx.scratch_bytes()
        assert all(n > 0 for n in sizes), dict(zip(SLOT, sizes))
        ctx.paint_scratch(0xA5)
        for name, which in SLOT.items():
            n = sizes[which]
            if which < 5:
                head, tail = ctx.scratch_read(which, 0, min(n, 4096)), ctx.scratch_read(which, n - min(n, 4096), min(n, 4096))
                assert (head == 0xA5).all() and (tail == 0xA5).all(), name
            else:                                        # several buffers read as one run: every byte of every one of them
                assert n < (64 << 20), (name, n)
                assert (ctx.scratch_read(which, 0, n) == 0xA5).all(), name
            with pytest.raises(afv._lib.AfvError):
                ctx.scratch_read(which, n, 1)
        assert ctx.scratch_bytes() == sizes and ctx.rest_words() == 0
        # the painted pair buffers and column slices are not read: the same answers again
        m2, nm2 = wide.match_pairs([0], [1], 75.0, 0.6)
        assert nm2[0] == wn and np.array_equal(m2, m) and ctx.rest_words() == 0
        got = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
        from test_gpu_poseopt import assert_equal
        assert_equal(got, s.run(inf=rig.inf), "after the paint")
        pts = np.ascontiguousarray(s.pts, np.int32)
        staged = ctx.scratch_read("d_match", 0, pts.nbytes)
        assert staged.tobytes() == pts.tobytes() != b"\xa5" * pts.nbytes, "the first input of afv_frame_pose_optimize is not at the head of d_match"
        assert ctx.scratch_read("h_stage", 0, pts.nbytes).tobytes() == pts.tobytes()
        tail = ctx.scratch_read("d_match", sizes[0] - 4096, 4096)
        assert (tail == 0xA5).all(), "a small call wrote the far end of d_match"
    finally:
        for o in (table, wide):
            if o is not None:
                o.close()
        rig.close()


_alone = {}


def alone(afv, oracle, chain):
    """the bytes of every step of a chain, each on a fresh context of its own: what every other run must repeat (once per session)"""
    if chain not in _alone:
        out = []
        for step in SC.CHAINS[chain][1]:
            ctx = afv.Context(**SC.CTX)
            try:
                out.append(step(afv, ctx, oracle))
                assert ctx.rest_words() == 0, (chain, step.__name__)
            finally:
                ctx.close()
        _alone[chain] = out
    return _alone[chain]


def run_chain(afv, oracle, chain, ctx, paint=None):
    """the largest step of the chain on a larger scene first, then the chain on that one context -> the bytes of its steps"""
    first, steps = SC.CHAINS[chain]
    first(afv, ctx, oracle)
    grown = ctx.scratch_bytes()[:5]
    out = []
    for step in steps:
        if paint is not None:
            ctx.paint_scratch(paint)
        out.append(step(afv, ctx, oracle))
    # no step outgrew what the first call left: the chain ran inside buffers that were larger than it needs and stale from end to end
    assert ctx.scratch_bytes()[:2] == grown[:2], (chain, "a step of the chain grew d_match / h_stage", grown, ctx.scratch_bytes())
    return out


@pytest.mark.parametrize("chain", sorted(SC.CHAINS))
def test_role_chain(afv, oracle, fresh, chain):
    """different layouts over the same bytes: every step alone on a fresh context, the chain on one context whose buffers an earlier,
    larger call of the chain's largest step has grown and filled, and the same with the scratch painted 0xFF between the steps.  Every
    step holds its answer to its restatement; the three runs must agree byte for byte"""
    want = alone(afv, oracle, chain)
    names = [s.__name__ for s in SC.CHAINS[chain][1]]
    for what, paint in (("chained", None), ("chained, painted 0xFF between the steps", 0xFF)):
        ctx = fresh()
        got = run_chain(afv, oracle, chain, ctx, paint)
        for name, g, w in zip(names, got, want):
            assert g == w, (chain, what, name, "differs from the step alone on a fresh context")
        assert ctx.rest_words() == 0, (chain, what)
    assert len(set(want)) == len(want)                  # the steps are different calls


def test_three_roles_at_once(afv, oracle):
    """a net, not a proof: tracking, local mapping and loop closing on three threads, each with a context of its own that is made and
    closed inside the thread every round together with its tables, stores and frames; every step of every round against the serial bytes.
    AFV_STRESS_ROUNDS sets the rounds"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rounds = int(os.environ.get("AFV_STRESS_ROUNDS", "5"))
    chains = sorted(SC.CHAINS)
    want = {c: alone(afv, oracle, c) for c in chains}
    bad, errors = [], []
    start = threading.Barrier(len(chains))

    def worker(chain):
        try:
            start.wait()
            for r in range(rounds):
                ctx = afv.Context(**SC.CTX)
                try:
                    got = run_chain(afv, oracle, chain, ctx)
                    rest = ctx.rest_words()
                finally:
                    ctx.close()
                for step, g, w in zip(SC.CHAINS[chain][1], got, want[chain]):
                    if g != w:
                        bad.append((chain, r, step.__name__))
                if rest:
                    bad.append((chain, r, "rest words", rest))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append((chain, repr(e)))
            start.abort()

    t0 = time.perf_counter()
    threads = [threading.Thread(target=worker, args=(c,), name=c) for c in chains]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    print("three roles, %d rounds: %.2f s" % (rounds, time.perf_counter() - t0))
    assert not errors, errors
    assert not bad, "thread, round, step that differ from the serial bytes: %r" % (bad[:10],)

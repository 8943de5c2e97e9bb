"""-m gpu: afv_set_split_schedule changes WHEN the kernels of a split batch run, never what they compute.  For both schedules and for chunk
counts 2, 3, 5, 6 and one above the frame count (empty chunks), on a 333 x 251 and a 160 x 120 context with 7 and 12 frames and
set_split_threshold(2): keypoints, descriptors and counts of extract_batch_device and match / nmatches of match_pairs_device (pairs t, t - 1)
are byte-equal to the unsplit run (set_split_threshold(1 << 30)); two calls back to back without a synchronise give the same bytes; and on a
caller stream other than the default a torch reduction of the counts enqueued right behind the call sees the final values.
Bar: 0 differing bytes (up to each frame's count: rows behind it are not written)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = {"333x251": (333, 251, 8), "160x120": (160, 120, 4)}   # width, height, levels
NFRAMES = (7, 12)


class _Case:
    def __init__(self, afv, w, h, nlevels, nf):
        import torch
        self.afv, self.nf, self.torch = afv, nf, torch
        self.ctx = afv.Context(nlevels=nlevels, max_width=w, max_height=h, max_batch=nf)
        pitch = (w + 3) // 4 * 4                                 # the device entry point takes 4-byte aligned row strides
        host = np.zeros((nf, h, pitch), np.uint8)
        for i in range(nf):
            host[i, :, :w] = afv.synth.corners_frame(40 + i, w, h)
        self.frames = torch.from_numpy(host).cuda()[:, :, :w]
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        self.m = afv.FeatureMatcher(0.6, True, ctx=self.ctx)
        self.pa = torch.arange(nf, dtype=torch.int32, device="cuda")
        self.pb = (self.pa + nf - 1) % nf
        self.stream = torch.cuda.Stream()
        self.ctx.set_split_threshold(1 << 30)
        self.ref = self.run(self.fresh())
        assert self.ref[2].min() > 0, "the scene must give every frame keypoints"

    def fresh(self):
        torch, nf, cap = self.torch, self.nf, self.ctx.cap
        return (torch.zeros((nf, cap, 7), dtype=torch.float32, device="cuda"), torch.zeros((nf, cap, 32), dtype=torch.uint8, device="cuda"),
                torch.zeros((nf,), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda"),
                torch.zeros((nf, cap), dtype=torch.int32, device="cuda"), torch.zeros((nf,), dtype=torch.int32, device="cuda"))

    def enqueue(self, bufs, stream=None):
        kps, desc, n, st, match, nm = bufs
        self.ctx.extract_batch_device(self.frames, kps, desc, n, st, self.ctx.cap, stream=stream)
        self.m.match_pairs_device(desc, kps, n, self.pa, self.pb, th_low=75.0, check_orientation=True, match=match, nmatches=nm, stream=stream)

    def collect(self, bufs):
        self.torch.cuda.synchronize()
        kps, desc, n, st, match, nm = (b.cpu().numpy() for b in bufs)
        assert int(st[0]) == 0
        rows = [(kps[i, :n[i]].tobytes(), desc[i, :n[i]].tobytes(), match[i, :n[i]].tobytes()) for i in range(self.nf)]
        return rows, nm.tobytes(), n

    def run(self, bufs, stream=None):
        self.enqueue(bufs, stream)
        return self.collect(bufs)

    def same(self, got):
        return got[0] == self.ref[0] and got[1] == self.ref[1] and np.array_equal(got[2], self.ref[2])


@pytest.fixture(scope="module")
def cases(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(size, nf):
        if (size, nf) not in made:
            made[(size, nf)] = _Case(afv, *SIZES[size], nf)
        return made[(size, nf)]
    yield get
    for c in made.values():
        c.ctx.close()


def test_schedule_setter_takes_0_and_1(cases):
    ctx = cases("160x120", 7).ctx
    for bad in (-1, 2, 8):
        with pytest.raises(Exception):
            ctx.set_split_schedule(bad)
    ctx.set_split_schedule(0)
    ctx.set_split_schedule(1)


@pytest.mark.parametrize("chunks", ["2", "3", "5", "6", "n+1"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nf", NFRAMES)
@pytest.mark.parametrize("size", sorted(SIZES))
def test_split_schedules_give_the_unsplit_bytes(cases, size, nf, mode, chunks):
    import torch
    c = cases(size, nf)
    ctx = c.ctx
    ctx.set_split_threshold(2)
    ctx.set_split_schedule(mode)
    ctx.set_split_chunks(nf + 1 if chunks == "n+1" else int(chunks))
    try:
        # one call
        assert c.same(c.run(c.fresh()))
        # two calls back to back on the context's own stream order, nothing between them: the second must not overtake the first's tail
        a, b = c.fresh(), c.fresh()
        c.enqueue(a)
        c.enqueue(b)
        assert c.same(c.collect(a)) and c.same(c.collect(b))
        # a caller stream of its own: what it enqueues behind the call sees the final counts
        bufs = c.fresh()
        torch.cuda.synchronize()
        with torch.cuda.stream(c.stream):
            c.enqueue(bufs)
            total, total_m = bufs[2].sum(), bufs[5].sum()
        c.stream.synchronize()
        assert int(total.item()) == int(c.ref[2].sum()) and int(total_m.item()) == int(np.frombuffer(c.ref[1], np.int32).sum())
        assert c.same(c.collect(bufs))
    finally:
        ctx.set_split_threshold(1 << 30)
        ctx.set_split_schedule(1)
        ctx.set_split_chunks(0)

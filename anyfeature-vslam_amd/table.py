"""Keyframe descriptor table resident in HBM + RCCL communicator (mirror of the afv_table_* / afv_comm_* C-ABI).

Reference call shape: LoopClosing::ComputeSim3 (LoopClosing.cc:255-281) / Tracking::Relocalization (Tracking.cc:1162-1182)
run SearchByBoW once per candidate keyframe, LocalMapping::CreateNewMapPoints (LocalMapping.cc:238-297)
SearchForTriangulation per neighbour; the descriptors they re-read are const after keyframe construction
(KeyFrame.h:190).  `DescriptorTable` keeps them on the device; batches of (slot a, slot b) jobs run against it.
Plumbing only: every method is one C-ABI call.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import TableTriJob, TriPointsJob, ptr


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


class Communicator:
    """afv_comm: RCCL communicator, one process per GPU.  `exchange_id(id_bytes_or_None) -> id_bytes` moves rank 0's
    128-byte id to every rank through any host channel (torch.distributed object broadcast, a file, a socket)."""

    def __init__(self, ctx, rank, world, exchange_id):
        self.ctx, self.lib = ctx, ctx.lib
        self.rank, self.world = int(rank), int(world)
        ident = None
        if self.rank == 0:
            buf = (C.c_uint8 * 128)()
            ctx.check(self.lib.afv_comm_unique_id(buf), "afv_comm_unique_id")
            ident = bytes(buf)
        ident = exchange_id(ident)
        assert isinstance(ident, (bytes, bytearray)) and len(ident) == 128
        h = C.c_void_p()
        ctx.check(self.lib.afv_comm_create(ctx.handle, (C.c_uint8 * 128).from_buffer_copy(ident), self.world, self.rank, C.byref(h)),
                  "afv_comm_create")
        self.handle = h

    def broadcast(self, tensor, root=0, stream=None):
        """in-place broadcast of a contiguous CUDA tensor (ncclBroadcast over xGMI), asynchronous on the context's stream"""
        assert tensor.is_cuda and tensor.is_contiguous()
        self.ctx.check(self.lib.afv_comm_broadcast(self.handle, tensor.data_ptr(), tensor.numel() * tensor.element_size(), int(root), stream),
                       "afv_comm_broadcast")

    def allgather(self, send, recv, stream=None):
        assert send.is_cuda and recv.is_cuda and send.is_contiguous() and recv.is_contiguous()
        nbytes = send.numel() * send.element_size()
        assert recv.numel() * recv.element_size() == nbytes * self.world
        self.ctx.check(self.lib.afv_comm_allgather(self.handle, send.data_ptr(), recv.data_ptr(), nbytes, stream), "afv_comm_allgather")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.afv_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_range(n_units, rank, world):
    """afv_shard_range: contiguous block partition (same rule as dist.shard_range, evaluated by the library)"""
    lo, hi = C.c_long(), C.c_long()
    _lib.load().afv_shard_range(int(n_units), int(rank), int(world), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class DescriptorTable:
    """`desc_bytes`: width of the binary rows, 1 .. 64 (32 = ORB32, 61 = AKAZE61, 48 = BRISK48 ...).  The device keeps them zero-padded to
    `pitch` = 32 (up to 32 bytes) or 64 bytes; host arrays in and out are `desc_bytes` wide.
    `float_dim` (instead of `desc_bytes`): a table of float rows (128 = SIFT128, 64 = SURF64 / KAZE64 ...), a multiple of 4 from 4 to 1024;
    host arrays and the device view are float32 of shape (n, float_dim), `desc_bytes` = `pitch` = 4 * float_dim, distances are L2^2."""

    def __init__(self, ctx, nsets, cap, desc_bytes=None, float_dim=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.nsets, self.cap = int(nsets), int(cap)
        if desc_bytes is not None and float_dim is not None:
            raise ValueError("desc_bytes and float_dim exclude each other: a table holds binary rows or float rows")
        self.float_dim = 0
        if float_dim is not None:
            if (isinstance(float_dim, bool) or not isinstance(float_dim, (int, np.integer)) or not 4 <= int(float_dim) <= 1024
                    or int(float_dim) % 4):
                raise ValueError("float_dim must be a multiple of 4 in 4..1024, got %r" % (float_dim,))
            self.float_dim = int(float_dim)
            self.desc_bytes = self.pitch = 4 * self.float_dim
            h = C.c_void_p()
            ctx.check(self.lib.afv_table_create_f32(ctx.handle, self.nsets, self.cap, self.float_dim, C.byref(h)), "afv_table_create_f32")
            self.handle = h
            return
        if desc_bytes is None:
            desc_bytes = 32
        if isinstance(desc_bytes, bool) or not isinstance(desc_bytes, (int, np.integer)) or not 1 <= int(desc_bytes) <= 64:
            raise ValueError("desc_bytes must be an integer in 1..64, got %r" % (desc_bytes,))
        self.desc_bytes = int(desc_bytes)
        self.pitch = 32 if self.desc_bytes <= 32 else 64
        h = C.c_void_p()
        if self.desc_bytes == 32:
            ctx.check(self.lib.afv_table_create(ctx.handle, self.nsets, self.cap, C.byref(h)), "afv_table_create")
        else:
            ctx.check(self.lib.afv_table_create_bytes(ctx.handle, self.nsets, self.cap, self.desc_bytes, C.byref(h)), "afv_table_create_bytes")
        self.handle = h

    def _rows(self, desc, what):
        """host rows as a contiguous (n, desc_bytes) uint8 array - (n, float_dim) float32 for a float table; a row of another width or
        kind raises before any library call"""
        a = np.asarray(desc)
        if self.float_dim:
            if a.ndim != 2 or a.shape[1] != self.float_dim or a.dtype != np.float32:
                raise ValueError("%s: rows must be (n, %d) float32 for this table, got shape %s %s" % (what, self.float_dim, a.shape, a.dtype))
            return np.ascontiguousarray(a)
        if a.ndim != 2 or a.shape[1] != self.desc_bytes:
            raise ValueError("%s: rows must be (n, %d) uint8 for this table, got shape %s" % (what, self.desc_bytes, a.shape))
        return np.ascontiguousarray(a, np.uint8)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.afv_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- filling ----
    def set(self, slot, desc, angles=None):
        if self.desc_bytes == 32 and not self.float_dim:
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        else:
            desc = self._rows(desc, "DescriptorTable.set")
        ang = None if angles is None else np.ascontiguousarray(angles, np.float32)
        self.ctx.check(self.lib.afv_table_set(self.handle, int(slot), ptr(desc), ptr(ang), len(desc)), "afv_table_set")

    def set_featvec(self, slot, node_id, seg_ptr, seg_idx):
        node_id, seg_ptr, seg_idx = _i32(node_id), _i32(seg_ptr), _i32(seg_idx)
        self.ctx.check(self.lib.afv_table_set_featvec(self.handle, int(slot), ptr(node_id), ptr(seg_ptr), ptr(seg_idx), len(node_id)),
                       "afv_table_set_featvec")

    def set_bowvec(self, slot, word, value):
        """KeyFrame::mBowVec of a slot: word ids ascending and unique, values float64 (Vocabulary.transform / Frame.bowvec)"""
        word, value = _i32(word), np.ascontiguousarray(value, np.float64)
        if len(word) != len(value):
            raise ValueError("DescriptorTable.set_bowvec: %d words, %d values" % (len(word), len(value)))
        self.ctx.check(self.lib.afv_table_set_bowvec(self.handle, int(slot), ptr(word), ptr(value), len(word)), "afv_table_set_bowvec")

    def set_geometry(self, slot, x, y, sigma2, u_right=None):
        """mvKeysUn positions and GetKeyPt1DSigma2 of a slot; u_right = KeyFrame::mvuRight of a stereo keyframe (None: monocular)"""
        x, y, s = (np.ascontiguousarray(v, np.float32) for v in (x, y, sigma2))
        self.ctx.check(self.lib.afv_table_set_geometry(self.handle, int(slot), ptr(x), ptr(y), ptr(s)), "afv_table_set_geometry")
        if u_right is not None:
            u = np.ascontiguousarray(u_right, np.float32)
            self.ctx.check(self.lib.afv_table_set_u_right(self.handle, int(slot), ptr(u)), "afv_table_set_u_right")

    def set_inf(self, slot, inf):
        """KeyFrame::GetKeyPt2DInf of a slot (the information of feature i is inf[i] * I), after set_geometry: what OptimizeSim3 reads"""
        v = np.ascontiguousarray(inf, np.float32)
        self.ctx.check(self.lib.afv_table_set_inf(self.handle, int(slot), ptr(v)), "afv_table_set_inf")

    def set_scale(self, slot, size, depth=None, x_dist=None, y_dist=None):
        """KeyFrame::GetKeyPtSize, mvDepth and the distorted mvKeys of a slot, after set_geometry: what triangulate reads next to the
        geometry.  depth None: -1 everywhere (monocular); x_dist / y_dist None (both or neither): the undistorted points"""
        a = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (size, depth, x_dist, y_dist)]
        self.ctx.check(self.lib.afv_table_set_scale(self.handle, int(slot), *[ptr(v) for v in a]), "afv_table_set_scale")

    def set_valid(self, slot, valid):
        """valid[i] = feature i has a good map point (None = all valid); honoured by match_bow"""
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        self.ctx.check(self.lib.afv_table_set_valid(self.handle, int(slot), ptr(v)), "afv_table_set_valid")

    def device_views(self):
        """zero-copy torch views of the table: desc uint8 [nsets, cap, pitch] (rows zero-padded from desc_bytes), angle float32
        [nsets, cap], n int32 [nsets]; a float table: desc float32 [nsets, cap, float_dim]"""
        import torch
        d, a, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.lib.afv_table_device_ptrs(self.handle, C.byref(d), C.byref(a), C.byref(n)))
        dev = torch.device("cuda", self.ctx.device)

        def view(p, nbytes, dtype, shape):
            class _Holder:  # __cuda_array_interface__ carrier; the table owns the memory
                pass
            h = _Holder()
            typestr = {torch.uint8: "|u1", torch.float32: "<f4", torch.int32: "<i4"}[dtype]
            h.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (p.value, False), "version": 2}
            return torch.as_tensor(h, device=dev)
        return (view(d, self.nsets * self.cap * self.pitch, torch.float32, (self.nsets, self.cap, self.float_dim)) if self.float_dim else
                view(d, self.nsets * self.cap * self.pitch, torch.uint8, (self.nsets, self.cap, self.pitch)),
                view(a, self.nsets * self.cap * 4, torch.float32, (self.nsets, self.cap)),
                view(n, self.nsets * 4, torch.int32, (self.nsets,)))

    def upload(self, table, angles, counts):
        """fill every slot from host arrays [nsets, cap, desc_bytes] / [nsets, cap] / [nsets]: three bulk copies through the
        zero-copy views when torch can wrap the pointers, else one afv_table_set per slot"""
        if self.float_dim:
            t_dev = np.asarray(table)
            if t_dev.shape != (self.nsets, self.cap, self.float_dim) or t_dev.dtype != np.float32:
                raise ValueError("DescriptorTable.upload: table must be (%d, %d, %d) float32, got shape %s %s"
                                 % (self.nsets, self.cap, self.float_dim, t_dev.shape, t_dev.dtype))
        elif self.desc_bytes != 32:
            t = np.asarray(table)
            if t.shape != (self.nsets, self.cap, self.desc_bytes):
                raise ValueError("DescriptorTable.upload: table must be (%d, %d, %d) uint8, got shape %s" % (self.nsets, self.cap, self.desc_bytes, t.shape))
            if self.pitch != self.desc_bytes:  # the device rows carry zero padding
                padded = np.zeros((self.nsets, self.cap, self.pitch), np.uint8)
                padded[:, :, :self.desc_bytes] = t
                t_dev = padded
            else:
                t_dev = t
        else:
            t_dev = table
        try:
            import torch
            d, a, n = self.device_views()
            d.copy_(torch.from_numpy(np.ascontiguousarray(t_dev, np.float32 if self.float_dim else np.uint8)))
            a.copy_(torch.from_numpy(np.ascontiguousarray(angles, np.float32)))
            n.copy_(torch.from_numpy(np.ascontiguousarray(counts, np.int32)))
            torch.cuda.synchronize(d.device)
            self.sync_counts()
        except (ImportError, TypeError, RuntimeError):
            for k in range(self.nsets):
                self.set(k, table[k, :counts[k]], angles[k, :counts[k]])

    def sync_counts(self):
        self.ctx.check(self.lib.afv_table_sync_counts(self.handle), "afv_table_sync_counts")

    # ---- replication ----
    def broadcast(self, comm, root=0):
        """one RCCL broadcast per array + one for the replica image (FeatureVector structure, per-slot flags); returns the device time
        of the broadcasts in ms"""
        ms = C.c_float(0.0)
        self.ctx.check(self.lib.afv_table_broadcast(comm.handle, self.handle, int(root), C.byref(ms)), "afv_table_broadcast")
        return float(ms.value)

    def clone_into(self, other):
        """replica without a communicator: everything this table holds, rebuilt in `other` the way a broadcast receiver does"""
        other.ctx.check(self.lib.afv_table_clone(self.handle, other.handle), "afv_table_clone")
        return other

    # ---- matching ----
    def match_pairs(self, pair_a, pair_b, th_low, nnratio, check_orientation=True, want_matches=True):
        """brute-force SearchByBoW(KF,KF) per pair; host arrays in, host arrays out"""
        pa, pb = _i32(pair_a), _i32(pair_b)
        n = len(pa)
        m = np.empty((n, self.cap), np.int32) if want_matches else None
        nm = np.zeros(n, np.int32)
        self.ctx.check(self.lib.afv_table_match_pairs(self.handle, ptr(pa), ptr(pb), n, float(th_low), float(nnratio), int(bool(check_orientation)),
                                                      ptr(m), ptr(nm)), "afv_table_match_pairs")
        return m, nm

    def match_pairs_device(self, pair_a, pair_b, th_low, nnratio, check_orientation=True, match=None, nmatches=None, stream=None):
        """device tensors in (int32 pair lists), device tensors out; asynchronous on torch's current stream"""
        import torch
        n = pair_a.numel()
        if match is None:
            match = torch.empty((n, self.cap), dtype=torch.int32, device=pair_a.device)
        if nmatches is None:
            nmatches = torch.empty((n,), dtype=torch.int32, device=pair_a.device)
        rc = _lib.launch_ordered(self.ctx, pair_a.device, stream, lambda s: self.lib.afv_table_match_pairs_device(
            self.handle, pair_a.data_ptr(), pair_b.data_ptr(), n, float(th_low), float(nnratio), int(bool(check_orientation)),
            match.data_ptr(), nmatches.data_ptr(), s), (pair_a, pair_b, match, nmatches))
        self.ctx.check(rc,
                       "afv_table_match_pairs_device")
        return match, nmatches

    def match_bow(self, pair_a, pair_b, th_low, nnratio, check_orientation=True, want_matches=True):
        """BoW-guided SearchByBoW(KF,KF) per pair over the stored FeatureVectors"""
        pa, pb = _i32(pair_a), _i32(pair_b)
        n = len(pa)
        m = np.empty((n, self.cap), np.int32) if want_matches else None
        nm = np.zeros(n, np.int32)
        self.ctx.check(self.lib.afv_table_match_bow(self.handle, ptr(pa), ptr(pb), n, float(th_low), float(nnratio), int(bool(check_orientation)),
                                                    ptr(m), ptr(nm)), "afv_table_match_bow")
        return m, nm

    def match_bow_frame(self, slots, frame, th_low, nnratio, check_orientation=True, want_matches=True):
        """relocalisation batch: SearchByBoW(KF, Frame) of ONE frame (a matcher.FeatureView: descriptors, FeatureVector, angles) against
        the keyframes in `slots`.  Returns match_f[nslots, frame.N] (keyframe feature per frame feature, -1 = none) and nmatches[nslots]"""
        from ._lib import FrameView
        sl = _i32(slots)
        if self.desc_bytes == 32 and not self.float_dim:
            desc = np.ascontiguousarray(frame.descriptors, np.uint8).reshape(-1, 32)
        else:
            desc = self._rows(frame.descriptors, "DescriptorTable.match_bow_frame")
        ids, sp, flat, nn = frame.csr()
        ids, sp, flat = _i32(ids), _i32(sp), _i32(flat)
        ang = None if frame.angles is None else np.ascontiguousarray(frame.angles, np.float32)
        fv = FrameView(desc.ctypes.data if len(desc) else None, len(desc), None if ang is None else ang.ctypes.data,
                       ids.ctypes.data if nn else None, sp.ctypes.data if nn else None, flat.ctypes.data if nn else None, int(nn))
        m = np.empty((len(sl), len(desc)), np.int32) if want_matches else None
        nm = np.zeros(len(sl), np.int32)
        self.ctx.check(self.lib.afv_table_match_bow_frame(self.handle, ptr(sl), len(sl), C.byref(fv), float(th_low), float(nnratio),
                                                          int(bool(check_orientation)), ptr(m), ptr(nm)), "afv_table_match_bow_frame")
        return m, nm

    def set_from_frame(self, slot, frame):
        """KeyFrame::KeyFrame(Frame&) (KeyFrame.cc:36-60): a resident frame (frame.Frame) becomes keyframe `slot`, device to device"""
        self.ctx.check(self.lib.afv_table_set_from_frame(self.handle, int(slot), frame.handle), "afv_table_set_from_frame")

    def match_bow_frame_resident(self, slots, frame, th_low, nnratio, check_orientation=True, want_matches=True):
        """match_bow_frame with the frame side taken from a resident frame (frame.Frame after ComputeBoW): nothing of the frame travels"""
        sl = _i32(slots)
        m = np.empty((len(sl), frame.N), np.int32) if want_matches else None
        nm = np.zeros(len(sl), np.int32)
        self.ctx.check(self.lib.afv_table_match_bow_frame_h(self.handle, ptr(sl), len(sl), frame.handle, float(th_low), float(nnratio),
                                                            int(bool(check_orientation)), ptr(m), ptr(nm)), "afv_table_match_bow_frame_h")
        return m, nm

    def score_bow(self, queries, slot_mask=None, want_first=True):
        """words in common and Vocabulary::score (DBoW2 L1) of every query against the slots, one launch (afv_table_score_bow).
        queries: a list whose items are an int (the BowVector of that slot), a frame.Frame (its resident BowVector) or a (word, value)
        pair of host arrays.  slot_mask: uint8 [nsets] or None = every slot.  Returns common int32 [nq, nsets] (-1 = empty / masked /
        no BowVector), score float64 [nq, nsets], first_common int32 [nq, nsets] (None when want_first is False)"""
        from ._lib import BOW_QUERY_FRAME, BOW_QUERY_HOST, BOW_QUERY_SLOT, BowQuery
        nq = len(queries)
        rec = (BowQuery * max(nq, 1))()
        keep = []
        for r, q in zip(rec, queries):
            r.struct_size = C.sizeof(BowQuery)
            if isinstance(q, (int, np.integer)):
                r.kind, r.slot = BOW_QUERY_SLOT, int(q)
            elif hasattr(q, "handle"):
                r.kind, r.frame = BOW_QUERY_FRAME, q.handle
            else:
                word, value = _i32(q[0]), np.ascontiguousarray(q[1], np.float64)
                if len(word) != len(value):
                    raise ValueError("DescriptorTable.score_bow: %d words, %d values" % (len(word), len(value)))
                keep += [word, value]
                r.kind, r.n = BOW_QUERY_HOST, len(word)
                r.word, r.value = (word.ctypes.data, value.ctypes.data) if len(word) else (None, None)
        mask = None if slot_mask is None else np.ascontiguousarray(slot_mask, np.uint8)
        if mask is not None and mask.shape != (self.nsets,):
            raise ValueError("DescriptorTable.score_bow: slot_mask must have one byte per slot")
        common = np.zeros((nq, self.nsets), np.int32); score = np.zeros((nq, self.nsets), np.float64)
        first = np.zeros((nq, self.nsets), np.int32) if want_first else None
        self.ctx.check(self.lib.afv_table_score_bow(self.handle, rec, nq, ptr(mask), ptr(common), ptr(score), ptr(first)), "afv_table_score_bow")
        return common, score, first

    def match_triangulation(self, pair_a, pair_b, F12, epipoles, th_low, has_mp1=None, has_mp2=None, only_stereo=False):
        """SearchForTriangulation per pair.  F12: [npairs, 9] (row-major), epipoles: [npairs, 2]; has_mp1/2: per pair uint8
        arrays or None"""
        pa, pb = _i32(pair_a), _i32(pair_b)
        n = len(pa)
        F12 = np.ascontiguousarray(F12, np.float32).reshape(n, 9)
        ep = np.ascontiguousarray(epipoles, np.float32).reshape(n, 2)
        jobs = (TableTriJob * n)()
        keep = []
        for p in range(n):
            j = jobs[p]
            j.struct_size = C.sizeof(TableTriJob)
            for k in range(9):
                j.F12[k] = float(F12[p, k])
            j.ex, j.ey, j.th_low = float(ep[p, 0]), float(ep[p, 1]), float(th_low)
            j.only_stereo = int(bool(only_stereo))
            for name, src in (("has_mp1", has_mp1), ("has_mp2", has_mp2)):
                if src is not None and src[p] is not None:
                    a = np.ascontiguousarray(src[p], np.uint8)
                    keep.append(a)
                    setattr(j, name, a.ctypes.data)
        m = np.empty((n, self.cap), np.int32)
        nm = np.zeros(n, np.int32)
        self.ctx.check(self.lib.afv_table_match_triangulation(self.handle, ptr(pa), ptr(pb), jobs, n, ptr(m), ptr(nm)),
                       "afv_table_match_triangulation")
        return m, nm

    # ---- new map points ----
    @staticmethod
    def tri_points_jobs(cams_a, cams_b, ratio_factor, max_size1):
        """afv_tri_points_job records from per-pair camera dicts {Rcw, tcw, Ow, fx, fy, cx, cy, invfx, invfy, mb, mbf} (a = the current
        keyframe, b = the neighbour); ratio_factor = 1.5f * sizeTolerance, max_size1 = maxKeyPtSize of a: scalars or one per pair"""
        n = len(cams_a)
        rf = np.broadcast_to(np.asarray(ratio_factor, np.float32), (n,))
        ms = np.broadcast_to(np.asarray(max_size1, np.float32), (n,))
        jobs = (TriPointsJob * n)()
        for p, (a, b) in enumerate(zip(cams_a, cams_b)):
            j = jobs[p]
            j.struct_size = C.sizeof(TriPointsJob)
            for side, cam in (("1", a), ("2", b)):
                for name, key, cnt in (("Rcw", "Rcw", 9), ("tcw", "tcw", 3), ("Ow", "Ow", 3)):
                    v = np.asarray(cam[key], np.float32).reshape(cnt)
                    dst = getattr(j, name + side)
                    for k in range(cnt):
                        dst[k] = float(v[k])
                for key in ("fx", "fy", "cx", "cy", "invfx", "invfy"):
                    setattr(j, key + side, float(np.float32(cam[key])))
            j.mb1, j.mb2, j.mbf1 = float(np.float32(a["mb"])), float(np.float32(b["mb"])), float(np.float32(a["mbf"]))
            j.ratio_factor, j.max_size1 = float(rf[p]), float(ms[p])
        return jobs

    def triangulate(self, pair_a, pair_b, jobs, match12, points=None, first_id=0):
        """the match loop of CreateNewMapPoints (LocalMapping.cc:315-461) for every pair in one call: two launches, one wait.  jobs: a
        TriPointsJob array (tri_points_jobs); match12 [npairs, cap] as match_triangulation returns it; points: a MapPoints store that
        receives the new points from id first_id on, or None.  Returns status, route [npairs, cap] uint8 (_lib.TRI_STATUS / TRI_ROUTE),
        x3d [npairs, cap, 3], new_id [npairs, cap] (-1 = not accepted), n_new [npairs]"""
        pa, pb = _i32(pair_a), _i32(pair_b)
        n = len(pa)
        m = _i32(match12)
        if len(pb) != n or len(jobs) != n or m.shape != (n, self.cap):
            raise ValueError("DescriptorTable.triangulate: %d pairs need %d jobs and match12 of shape (%d, %d)" % (n, n, n, self.cap))
        status, route = np.zeros((n, self.cap), np.uint8), np.zeros((n, self.cap), np.uint8)
        x3d = np.zeros((n, self.cap, 3), np.float32)
        new_id, n_new = np.full((n, self.cap), -1, np.int32), np.zeros(n, np.int32)
        self.ctx.check(self.lib.afv_table_triangulate(self.handle, ptr(pa), ptr(pb), jobs, n, ptr(m), None if points is None else points.handle,
                                                      int(first_id), ptr(status), ptr(route), ptr(x3d), ptr(new_id), ptr(n_new)),
                       "afv_table_triangulate")
        return status, route, x3d, new_id, n_new

    def CreateNewMapPoints(self, points, cur, neighbours, cams, F12, epipoles, th_low, has_mp, first_id, only_stereo=False):
        """the neighbour loop of LocalMapping::CreateNewMapPoints (LocalMapping.cc:265-472) as the reference runs it: one neighbour at a
        time, each with one match_triangulation call and one triangulate call; between neighbours the features of `cur` and of that
        neighbour that received a point are marked in the host masks, so a feature of `cur` gets at most one point.
        cur: the slot of the current keyframe; neighbours: the slots that survived the caller's baseline tests (:272-289), in order;
        cams: {slot: camera dict as tri_points_jobs takes it, plus "ratio_factor" and "max_size" for cur's}; F12 [nn, 9], epipoles [nn, 2]
        per neighbour; has_mp: {slot: uint8 mask "already has a map point"} - the masks are UPDATED in place.
        Returns a list of (id, [(slot, feature), (slot, feature)]) observations in creation order.
        All neighbours can be batched into ONE triangulate call (it takes up to 64 pairs); the masks are then those of before the first
        neighbour, and a stale mask no longer gives the reference's answer: a feature may receive a point from several neighbours."""
        F12 = np.ascontiguousarray(F12, np.float32).reshape(len(neighbours), 9)
        ep = np.ascontiguousarray(epipoles, np.float32).reshape(len(neighbours), 2)
        out = []
        nid = int(first_id)
        for k, nb in enumerate(neighbours):
            m, _ = self.match_triangulation([cur], [nb], F12[k:k + 1], ep[k:k + 1], th_low, [has_mp[cur]], [has_mp[nb]], only_stereo)
            jobs = self.tri_points_jobs([cams[cur]], [cams[nb]], cams[cur]["ratio_factor"], cams[cur]["max_size"])
            _, _, _, new_id, _ = self.triangulate([cur], [nb], jobs, m, points, nid)
            for i in np.nonzero(new_id[0] >= 0)[0]:
                j = int(m[0, i])
                out.append((int(new_id[0, i]), [(int(cur), int(i)), (int(nb), j)]))
                has_mp[cur][i] = 1
                has_mp[nb][j] = 1
                nid += 1
        return out

    def create_new_points(self, cur, neighbours, F12, epipoles, th_low, jobs, has_mp_cur, has_mp_nb, points=None, first_id=0, only_stereo=False):
        """the neighbour loop of CreateNewMapPoints in ONE call (afv_table_create_new_points): one upload, two launches per neighbour on the
        context's stream, one wait; the masks stay on the device between the neighbours.  F12 [nn, 9], epipoles [nn, 2]; jobs: a
        TriPointsJob array (tri_points_jobs, a = cur, b = neighbours[k]); has_mp_cur uint8 [cap] and has_mp_nb uint8 [nn, cap] (row k: the
        mask of neighbours[k]) are C-contiguous arrays UPDATED in place.
        Returns match12, status, route [nn, cap], x3d [nn, cap, 3], new_id [nn, cap], n_new [nn], n_done.  n_done < nn: the points of
        neighbour n_done did not fit the store (AFV_ECAPACITY): the neighbours before it stand, its rows and the later ones are empty -
        this is an answer, not an exception; every other error raises"""
        from ._lib import ECAPACITY
        nbs = _i32(neighbours)
        n = len(nbs)
        F12 = np.ascontiguousarray(F12, np.float32).reshape(n, 9)
        ep = np.ascontiguousarray(epipoles, np.float32).reshape(n, 2)
        for name, a, shape in (("has_mp_cur", has_mp_cur, (self.cap,)), ("has_mp_nb", has_mp_nb, (n, self.cap))):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == shape and a.flags.c_contiguous and a.flags.writeable):
                raise ValueError("DescriptorTable.create_new_points: %s must be a writeable C-contiguous uint8 array of shape %s" % (name, shape))
        if len(jobs) != n:
            raise ValueError("DescriptorTable.create_new_points: %d neighbours need %d jobs" % (n, n))
        search = (TableTriJob * max(n, 1))()
        for k in range(n):
            j = search[k]
            j.struct_size = C.sizeof(TableTriJob)
            for q in range(9):
                j.F12[q] = float(F12[k, q])
            j.ex, j.ey, j.th_low = float(ep[k, 0]), float(ep[k, 1]), float(th_low)
            j.only_stereo = int(bool(only_stereo))
        m = np.full((n, self.cap), -1, np.int32)
        status, route = np.zeros((n, self.cap), np.uint8), np.zeros((n, self.cap), np.uint8)
        x3d = np.zeros((n, self.cap, 3), np.float32)
        new_id, n_new = np.full((n, self.cap), -1, np.int32), np.zeros(n, np.int32)
        n_done = C.c_int32(0)
        rc = self.lib.afv_table_create_new_points(self.handle, int(cur), ptr(nbs), n, search, jobs, ptr(has_mp_cur), ptr(has_mp_nb),
                                                  None if points is None else points.handle, int(first_id), ptr(m), ptr(status), ptr(route),
                                                  ptr(x3d), ptr(new_id), ptr(n_new), C.byref(n_done))
        if rc != ECAPACITY:
            self.ctx.check(rc, "afv_table_create_new_points")
        return m, status, route, x3d, new_id, n_new, int(n_done.value)

    def CreateNewMapPointsChain(self, points, cur, neighbours, cams, F12, epipoles, th_low, has_mp, first_id, only_stereo=False):
        """CreateNewMapPoints with the same arguments, the same observation list and the same in-place update of the masks, from ONE
        create_new_points call instead of two calls per neighbour.  A store that cannot take the points of neighbour k raises AfvError
        (ECAPACITY) as the loop does at its k-th triangulate call; the masks then hold what neighbours 0 .. k - 1 marked"""
        from ._lib import AfvError, ECAPACITY
        nn = len(neighbours)
        jobs = self.tri_points_jobs([cams[cur]] * nn, [cams[nb] for nb in neighbours], cams[cur]["ratio_factor"], cams[cur]["max_size"])
        m_cur = np.zeros(self.cap, np.uint8)
        m_nb = np.zeros((nn, self.cap), np.uint8)
        m_cur[:len(has_mp[cur])] = has_mp[cur]
        for k, nb in enumerate(neighbours):
            m_nb[k, :len(has_mp[nb])] = has_mp[nb]
        m, _, _, _, new_id, _, n_done = self.create_new_points(cur, neighbours, F12, epipoles, th_low, jobs, m_cur, m_nb, points, first_id, only_stereo)
        out = []
        for k, nb in enumerate(neighbours[:n_done]):
            for i in np.nonzero(new_id[k] >= 0)[0]:
                out.append((int(new_id[k, i]), [(int(cur), int(i)), (int(nb), int(m[k, i]))]))
            has_mp[nb][:] = m_nb[k, :len(has_mp[nb])]
        has_mp[cur][:] = m_cur[:len(has_mp[cur])]
        if n_done < nn:
            raise AfvError(ECAPACITY, "afv_table_create_new_points " + self.lib.afv_last_error(self.ctx.handle).decode())
        return out

    # ---- fusing map points into keyframes of the table: Fuse (FeatureMatcher.cc:794-940, :942-1064) ----
    RADIUS_SCALE = 1.15  # FeatureMatcher's static radiusScale

    def set_camera(self, min_x, max_x, min_y, max_y, grid_cols, grid_rows, grid_inv_w, grid_inv_h):
        """the image bounds mnMinX .. mnMaxY and the grid of KeyFrame::GetFeaturesInArea for every slot (what FrameParams carries for a
        frame); the grid of a slot is built on the device on demand and kept until its geometry, its scale planes or this camera change"""
        cam = _lib.sized(_lib.TableCamera)
        cam.min_x, cam.max_x, cam.min_y, cam.max_y = float(min_x), float(max_x), float(min_y), float(max_y)
        cam.grid_cols, cam.grid_rows, cam.grid_inv_w, cam.grid_inv_h = int(grid_cols), int(grid_rows), float(grid_inv_w), float(grid_inv_h)
        self.ctx.check(self.lib.afv_table_set_camera(self.handle, C.byref(cam)), "afv_table_set_camera")

    def set_pose(self, slot, Rcw, tcw, Ow, fx, fy, cx, cy, mbf=0.0):
        """KeyFrame::SetPose of a slot + its intrinsics: Rcw [3, 3], tcw [3], Ow = -Rcw^T tcw as the host computes it (KeyFrame.cc:67-75)"""
        R = np.ascontiguousarray(Rcw, np.float32).reshape(9)
        t = np.ascontiguousarray(tcw, np.float32).reshape(3)
        o = np.ascontiguousarray(Ow, np.float32).reshape(3)
        self.ctx.check(self.lib.afv_table_set_pose(self.handle, int(slot), ptr(R), ptr(t), ptr(o), float(fx), float(fy), float(cx), float(cy),
                                                   float(mbf)), "afv_table_set_pose")

    def set_map_points(self, slot, ids):
        """KeyFrame::mvpMapPoints of a slot: one point id per feature, -1 = none"""
        ids = _i32(ids).reshape(-1)
        self.ctx.check(self.lib.afv_table_set_map_points(self.handle, int(slot), ptr(ids) if len(ids) else None), "afv_table_set_map_points")

    def get_map_points(self, slot, n):
        """the plane of a slot as the device holds it (tests): n = the slot's feature count"""
        out = np.full(max(int(n), 1), -1, np.int32)
        self.ctx.check(self.lib.afv_table_get_map_points(self.handle, int(slot), ptr(out)), "afv_table_get_map_points")
        return out[:int(n)].copy()

    def _fuse(self, points, targets, ids, radiusTh, th_low, use_inf_gate, poses):
        from .matcher import FeatureMatcher
        targets = [int(s) for s in targets]
        nt = len(targets)
        if nt and isinstance(ids, (list, tuple)) and len(ids) == nt and all(not np.isscalar(v) for v in ids):
            lists = [v if isinstance(v, np.ndarray) and v.dtype == np.int32 and v.flags.c_contiguous and v.ndim == 1 else _i32(v).reshape(-1)
                     for v in ids]
        else:
            shared = _i32(ids).reshape(-1)
            lists = [shared] * nt  # one pointer: the targets share one upload and one descriptor gather
        th = float(FeatureMatcher.TH_LOW if th_low is None else th_low)
        jobs = (_lib.TableFuseJob * max(nt, 1))()
        keep = []
        for k, (s, a) in enumerate(zip(targets, lists)):
            j = jobs[k]
            j.struct_size = C.sizeof(_lib.TableFuseJob)
            j.slot, j.nq = s, len(a)
            j.ids = a.ctypes.data if len(a) else None
            j.radius_th, j.radius_scale, j.th_low = float(radiusTh), float(np.float32(self.RADIUS_SCALE)), th
            j.use_inf_gate = int(bool(use_inf_gate))
            if poses is not None:
                R, t, Ow = poses[k]
                p = _lib.TableFusePose()
                for name, v, cnt in (("R", R, 9), ("t", t, 3), ("Ow", Ow, 3)):
                    v = np.asarray(v, np.float32).reshape(cnt)
                    dst = getattr(p, name)
                    for q in range(cnt):
                        dst[q] = float(v[q])
                keep.append(p)
                j.pose_override = C.pointer(p)
        total = sum(len(a) for a in lists)
        best, occ = np.full(max(total, 1), -1, np.int32), np.full(max(total, 1), -1, np.int32)
        status, nf = np.zeros(max(total, 1), np.uint8), np.zeros(max(nt, 1), np.int32)
        self.ctx.check(self.lib.afv_table_fuse_points(self.handle, points.handle, jobs, nt, ptr(best), ptr(occ), ptr(status), ptr(nf)),
                       "afv_table_fuse_points")
        cut = np.cumsum([0] + [len(a) for a in lists])
        split = lambda a: [a[cut[k]:cut[k + 1]].copy() for k in range(nt)]
        return split(best), split(occ), split(status), nf[:nt].copy()

    def FusePoints(self, points, targets, ids, radiusTh=3.0, th_low=None):
        """Fuse(pKF, vpMapPoints, th) (FeatureMatcher.cc:794-940) of the store's points `ids` into every slot of `targets` (up to 64) in ONE
        call.  ids: one list for all targets or a list per target, in the reference's iteration order, -1 allowed.
        Returns (best, occupant, status, nFused): lists with one array per target over its queries - the winning feature | -1, the point id
        the slot's plane holds there | -1, _lib.KFFUSE_STATUS - and nFused int32 [len(targets)], what the reference returns.
        SNAPSHOT: every target is answered against the store and the planes as they stand now; nothing is written.  The map surgery
        (AddObservation for status 4, Replace for 6) stays with the caller; one target per call with the updates in between gives the
        reference's sequential loop."""
        return self._fuse(points, targets, ids, radiusTh, th_low, True, None)

    @staticmethod
    def decompose_scw(Scw):
        """Rcw, tcw, Ow of a 4 x 4 Scw as Fuse(pKF, Scw, ...) writes them (FeatureMatcher.cc:954-958), in float, one rounding per
        operator: scw = the norm of row 0 of sRcw, Rcw = sRcw / scw, Ow = -Rcw^T tcw - and tcw is Scw's translation AS IT STANDS: the
        reference does not divide it by scw here (a kept quirk; it matters whenever s != 1)"""
        f32 = np.float32
        S = np.asarray(Scw, np.float32).reshape(4, 4)
        sR = S[:3, :3]
        scw = np.sqrt(f32(sR[0, 0] * sR[0, 0]) + (f32(sR[0, 1] * sR[0, 1]) + f32(sR[0, 2] * sR[0, 2])))
        R = (sR / f32(scw)).astype(np.float32)
        t = S[:3, 3].copy()
        Ow = np.array([f32(-R[0, k]) * t[0] + (f32(-R[1, k]) * t[1] + f32(-R[2, k]) * t[2]) for k in range(3)], np.float32)
        return R, t, Ow

    def FusePointsSim3(self, points, targets, Scw, ids, radiusTh=4.0, th_low=None):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (FeatureMatcher.cc:942-1064): as FusePoints, without the reprojection gates, each
        target seen through its own Scw (a 4 x 4 matrix per target, decomposed by decompose_scw).  Status 6 is vpReplacePoint[iMP]"""
        poses = [self.decompose_scw(S) for S in Scw]
        if len(poses) != len(targets):
            raise ValueError("DescriptorTable.FusePointsSim3: %d targets need %d Scw" % (len(targets), len(targets)))
        return self._fuse(points, targets, ids, radiusTh, th_low, False, poses)

    def SearchInNeighborsFuse(self, points, cur, targets, ids_cur, ids_of_target, on_fuse, radiusTh=3.0, th_low=None):
        """both halves of LocalMapping::SearchInNeighbors (LocalMapping.cc:505-533) with the reference's sequential semantics: one target
        per call, the caller's map surgery in between.  ids_cur(): the current keyframe's points at the time of the call (vpMapPointMatches
        is taken once, :507, so it is called once); ids_of_target(slot): GetMapPointMatches of a target when the second half reaches it.
        on_fuse(slot, ids, best, occupant, status) does AddObservation / Replace and must refresh the store flags and the planes it changed
        (set_flags, set_map_points).  The second half's candidate list is built with the mnFuseCandidateForKF de-duplication of :517-533.
        Returns (nFused per target, nFused of the second half)"""
        first = ids_cur()
        nf = []
        for s in targets:
            b, o, st, n = self.FusePoints(points, [s], first, radiusTh, th_low)
            on_fuse(int(s), np.asarray(first, np.int32), b[0], o[0], st[0])
            nf.append(int(n[0]))
        cand, seen = [], set()
        for s in targets:
            for i in ids_of_target(int(s)):
                i = int(i)
                if i < 0 or i in seen:  # (a bad point stays in the list: the store knows it and answers status 0, as :523 skips it)
                    continue
                seen.add(i)
                cand.append(i)
        b, o, st, n = self.FusePoints(points, [cur], cand, radiusTh, th_low)
        on_fuse(int(cur), np.asarray(cand, np.int32), b[0], o[0], st[0])
        return nf, int(n[0])

    def SearchAndFuse(self, points, corrected, Scw, loop_ids, on_fuse, radiusTh=4.0, th_low=None):
        """LoopClosing::SearchAndFuse (LoopClosing.cc:601-628): the loop map points into every corrected keyframe through its corrected
        Scw, one target per call; on_fuse(slot, ids, best, occupant, status) replaces the occupants of status 6 (:616-624).
        Returns nFused per keyframe"""
        ids = _i32(loop_ids).reshape(-1)
        nf = []
        for s, S in zip(corrected, Scw):
            b, o, st, n = self.FusePointsSim3(points, [s], [S], ids, radiusTh, th_low)
            on_fuse(int(s), ids, b[0], o[0], st[0])
            nf.append(int(n[0]))
        return nf

// afv_match_jobs.hip — host runtime of SearchByBoW(KF,KF), SearchByBoW(KF,F) and SearchForTriangulation (rows M2, M3, M4 of SURVEY.md).
// Every route (host arrays, keyframe-table slots, a table against a host frame view or a resident frame) describes the two sides of its
// jobs with MatchSide (afv_runtime.h) and calls afv_match_jobs_run: ONE place that checks FeatureVectors, merge-joins them, maps features
// to shared nodes, stages what lives on the host, fills the job records of k_match.hip, launches and fetches.
#include "afv_runtime.h"

// true when idx[0 .. total) (already checked to lie in [0, n)) holds an index twice.  O(total), a bitmap of n bits
static bool afv_featvec_lists_twice(const int32_t *idx, int total, int n) {
    std::vector<uint64_t> seen(((size_t)std::max(n, 0) + 63) / 64, 0);
    for (int i = 0; i < total; ++i) {
        uint64_t &w = seen[(size_t)idx[i] >> 6];
        const uint64_t bit = 1ull << (idx[i] & 63);
        if (w & bit) return true;
        w |= bit;
    }
    return false;
}

int afv_featvec_check(const int32_t *node_id, const int32_t *seg_ptr, const int32_t *seg_idx, int nnodes, int n) {
    if (nnodes == 0) return AFV_OK;
    if (seg_ptr[0] != 0) return AFV_EINVAL;
    for (int i = 0; i < nnodes; ++i) {
        if (seg_ptr[i + 1] < seg_ptr[i]) return AFV_EINVAL;
        if (i > 0 && node_id[i] <= node_id[i - 1]) return AFV_EINVAL;  // std::map order: strictly ascending node ids
    }
    const int total = seg_ptr[nnodes];
    if (total > n) return AFV_EINVAL;  // a feature sits in exactly one node
    for (int i = 0; i < total; ++i)
        if (seg_idx[i] < 0 || seg_idx[i] >= n) return AFV_EINVAL;
    return afv_featvec_lists_twice(seg_idx, total, n) ? AFV_EINVAL : AFV_OK;  // ... and is listed once: total <= n alone lets (0, 0) pass
}

// merge-join of two FeatureVectors (FeatureMatcher.cc:205-276): appends one (range1, range2) per shared node id
AFV_LOCAL void join_featvecs(const MatchSide &A, const MatchSide &B, bool whole_range, std::vector<Seg> &segs) {
    if (whole_range && (A.nnodes == 0 || B.nnodes == 0)) {
        segs.push_back(Seg{0, A.n, 0, B.n});
        return;
    }
    int a = 0, b = 0;
    while (a < A.nnodes && b < B.nnodes) {
        if (A.node_id[a] == B.node_id[b]) {
            segs.push_back(Seg{A.seg_ptr[a], A.seg_ptr[a + 1] - A.seg_ptr[a], B.seg_ptr[b], B.seg_ptr[b + 1] - B.seg_ptr[b]});
            ++a;
            ++b;
        } else if (A.node_id[a] < B.node_id[b]) {
            ++a;
        } else {
            ++b;
        }
    }
}

// feature of side 1 -> the shared node holding it, -1 = none (a feature sits in exactly one node of its FeatureVector).  An index outside
// [0, n1) is AFV_EINVAL.  Host-array jobs cannot get there: afv_featvec_check has seen every index of seg_idx[0 .. seg_ptr[nnodes]), the
// segments are sub-ranges of it, and the whole-range segment of a brute-force job names 0 .. n1 - 1; a table slot cannot either while
// afv_table_sync_counts drops the FeatureVector of a slot that shrank under it
AFV_LOCAL int build_row_seg(const MatchSide &A, const Seg *segs, int nseg, std::vector<int> &row_seg) {
    const int32_t *idx = A.on_device ? A.idx_host : A.idx;
    row_seg.assign((size_t)std::max(A.n, 1), -1);
    for (int s = 0; s < nseg; ++s)
        for (int r = 0; r < segs[s].n1; ++r) {
            const int f = idx ? idx[segs[s].s1 + r] : segs[s].s1 + r;
            if (f < 0 || f >= A.n) return AFV_EINVAL;
            row_seg[f] = s;
        }
    return AFV_OK;
}

namespace {
struct Ref {  // an array of a side on the device: its pointer, or where the blob holds the staged host copy
    const void *dev = nullptr;
    size_t off = 0;
    bool staged = false;
    template <class T>
    const T *at(const uint8_t *base) const { return reinterpret_cast<const T *>(staged ? base + off : dev); }
};
struct StagedSide {
    Ref rows, idx, valid, angle, x, y, sigma2, u_right;
};
Ref stage(Blob &b, const void *p, bool on_device, size_t bytes) {
    Ref r;
    if (!p) return r;
    if (on_device) {
        r.dev = p;
    } else {
        r.off = b.put(p, bytes);
        r.staged = true;
    }
    return r;
}
}  // namespace

int afv_match_jobs_run(afv_ctx *c, const MatchBatch &B, int32_t *out, int32_t *nmatches) {
    const int njobs = (int)B.jobs.size();
    HIPCHK(c, hipSetDevice(c->device));
    Blob b(c);
    std::vector<StagedSide> staged(B.sides.size());
    for (size_t i = 0; i < B.sides.size(); ++i) {
        const MatchSide &m = B.sides[i];
        StagedSide &s = staged[i];
        if (m.on_device) {
            s.rows.dev = m.rows;
        } else {  // rows narrower than the pitch are padded with zeros; float rows and rows at the pitch go as they are
            s.rows.off = (size_t)m.desc_bytes == (size_t)m.words * 4 ? b.put(m.rows, (size_t)m.n * m.desc_bytes)
                                                                     : put_desc(b, m.rows, m.n, m.desc_bytes, m.words);
            s.rows.staged = true;
        }
        s.idx = stage(b, m.idx, m.on_device, (size_t)(m.nnodes > 0 ? m.seg_ptr[m.nnodes] : 0) * 4);
        s.valid = stage(b, m.valid, m.valid_on_device, (size_t)m.n);
        if (B.tri) {
            s.x = stage(b, m.x, m.on_device, (size_t)m.n * 4);
            s.y = stage(b, m.y, m.on_device, (size_t)m.n * 4);
            s.sigma2 = stage(b, m.sigma2, m.on_device, (size_t)m.n * 4);
            s.u_right = stage(b, m.u_right, m.on_device, (size_t)m.n * 4);
        } else {
            s.angle = stage(b, m.angle, m.on_device, (size_t)m.n * 4);
        }
    }
    // per job: shared nodes (one task of the per-node kernel each), the row map of triangulation, the place of its output row
    std::vector<Seg> segs;
    std::vector<SegTask> tasks;
    std::vector<int> seg_first((size_t)njobs + 1, 0), out_pos((size_t)njobs, 0), row_seg;
    std::vector<size_t> rowseg_off((size_t)njobs, 0);
    bool per_node = B.per_node, any_ori = false;
    int max_n1 = 0;
    size_t total_out = 0;
    for (int p = 0; p < njobs; ++p) {
        const MatchJobSpec &j = B.jobs[p];
        const MatchSide &s1 = B.sides[j.side1], &s2 = B.sides[j.side2];
        const int first = seg_first[p];
        join_featvecs(s1, s2, B.whole_range, segs);
        const int nseg = (int)segs.size() - first;
        seg_first[p + 1] = first + nseg;
        if (!B.tri)
            for (int s = 0; s < nseg; ++s) tasks.push_back(SegTask{p, s});
        per_node = per_node || nseg > 1;
        any_ori = any_ori || j.check_ori;
        max_n1 = std::max(max_n1, s1.n);
        if (B.tri) {
            const int rc = build_row_seg(s1, segs.data() + first, nseg, row_seg);
            if (rc) return rc;
            rowseg_off[p] = b.put(row_seg.data(), row_seg.size() * sizeof(int));
        }
        out_pos[p] = (int)(B.out_stride ? (size_t)p * B.out_stride : total_out);
        total_out += B.out_stride ? (size_t)B.out_stride : (size_t)((!B.tri && j.mode == AFV_MATCH_KF_FRAME) ? s2.n : s1.n);
    }
    const bool seg_kernel = !B.tri && per_node;  // one wavefront per shared node; else (single-segment jobs) the ordered workgroup-per-job kernel
    const size_t job_bytes = B.tri ? sizeof(DevTriJob) : sizeof(DevMatchJob);
    const size_t segs_off = b.put(segs.data(), segs.size() * sizeof(Seg));
    const size_t tasks_off = b.put(tasks.data(), tasks.size() * sizeof(SegTask));
    const size_t jobs_off = b.reserve((size_t)njobs * job_bytes);
    const size_t binoff_off = b.put(out_pos.data(), seg_kernel ? (size_t)njobs * sizeof(int) : 0);  // a job's orientation bins sit where its output row does
    const size_t hist_off = b.reserve(seg_kernel ? (size_t)njobs * 32 * sizeof(int) : 0);
    const size_t nm_off = b.reserve((size_t)njobs * sizeof(int));  // the kernels accumulate: counters start at 0 ...
    const size_t in_bytes = b.h.size();
    const size_t out_off = b.reserve_scratch(std::max<size_t>(total_out, 1) * sizeof(int));  // ... and output rows at -1 (filled on the device)
    const size_t bins_off = b.reserve_scratch(seg_kernel ? std::max<size_t>(total_out, 1) : 0);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *base = c->d_match;
    for (int p = 0; p < njobs; ++p) {  // the only place that fills DevMatchJob / DevTriJob
        const MatchJobSpec &j = B.jobs[p];
        const MatchSide &s1 = B.sides[j.side1], &s2 = B.sides[j.side2];
        const StagedSide &g1 = staged[j.side1], &g2 = staged[j.side2];
        DevTriJob *T = B.tri ? reinterpret_cast<DevTriJob *>(b.h.data() + jobs_off) + p : nullptr;
        DevMatchJob &d = T ? T->m : reinterpret_cast<DevMatchJob *>(b.h.data() + jobs_off)[p];
        d.d1 = g1.rows.at<uint32_t>(base);
        d.d2 = g2.rows.at<uint32_t>(base);
        d.n1 = s1.n;
        d.n2 = s2.n;
        d.words = s1.fdim ? 0 : s1.words;
        d.fdim = s1.fdim;
        d.segs = reinterpret_cast<const Seg *>(base + segs_off) + seg_first[p];
        d.nseg = seg_first[p + 1] - seg_first[p];
        d.idx1 = g1.idx.at<int>(base);
        d.idx2 = g2.idx.at<int>(base);
        d.valid1 = g1.valid.at<uint8_t>(base);  // SearchByBoW: map point exists && !isBad(); triangulation: already has a map point => skip
        d.valid2 = g2.valid.at<uint8_t>(base);
        d.ang1 = g1.angle.at<float>(base);
        d.ang2 = g2.angle.at<float>(base);
        d.ang_stride = 1;
        d.th = j.th;
        d.ratio = j.ratio;
        d.check_ori = !B.tri && j.check_ori != 0;
        d.mode = B.tri ? (int)AFV_MATCH_KF_KF : j.mode;
        d.out = reinterpret_cast<int *>(base + out_off) + out_pos[p];
        d.nmatches = reinterpret_cast<int *>(base + nm_off) + p;
        if (!T) continue;
        T->x1 = g1.x.at<float>(base);
        T->y1 = g1.y.at<float>(base);
        T->x2 = g2.x.at<float>(base);
        T->y2 = g2.y.at<float>(base);
        T->sigma2_2 = g2.sigma2.at<float>(base);
        std::memcpy(T->F, j.F12, sizeof(T->F));
        T->ex = j.ex;
        T->ey = j.ey;
        T->row_seg = reinterpret_cast<const int *>(base + rowseg_off[p]);
        T->u_right1 = g1.u_right.at<float>(base);
        T->u_right2 = g2.u_right.at<float>(base);
        T->only_stereo = j.only_stereo != 0;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_match, b.h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
    if (total_out) HIPCHK(c, hipMemsetAsync(base + out_off, 0xff, total_out * sizeof(int), c->stream));  // -1
    if (B.tri)
        afv_launch_match_tri(reinterpret_cast<const DevTriJob *>(base + jobs_off), njobs, max_n1, c->stream);
    else if (!seg_kernel)
        afv_launch_match_bow(reinterpret_cast<const DevMatchJob *>(base + jobs_off), njobs, c->stream);
    else if (!tasks.empty())
        afv_launch_match_bow_seg(reinterpret_cast<const DevMatchJob *>(base + jobs_off), njobs, base + tasks_off, (int)tasks.size(),
                                 reinterpret_cast<int *>(base + hist_off), base + bins_off,
                                 reinterpret_cast<const int *>(base + binoff_off), any_ori ? 1 : 0, c->stream);
    HIPCHK(c, hipGetLastError());
    if (out) HIPCHK(c, b.fetch(out, out_off, total_out * sizeof(int), c->stream));
    HIPCHK(c, b.fetch(nmatches, nm_off, (size_t)njobs * sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.finish();
    return AFV_OK;
}

// plain brute-force KF-KF jobs over 32-byte descriptors take the two-phase path of the device pipeline (parallel top-k + ordered
// resolve), a different algorithm from the runner above: staged as a descriptor table of 2 sets per job
int afv_match_bow_plain32(afv_ctx *c, const afv_match_job *jobs, int njobs, int32_t *out, int32_t *nmatches, bool *taken) {
    bool eligible = true;
    int cap = 1;
    for (int i = 0; i < njobs; ++i) {
        const afv_match_job &j = jobs[i];
        eligible = eligible && (j.nnodes1 == 0 || j.nnodes2 == 0) && j.mode == AFV_MATCH_KF_KF && j.desc_bytes == 32 &&
                   !j.valid1 && !j.valid2 && j.n1 <= 4096 && j.n2 <= 4096;
        cap = std::max(cap, std::max(j.n1, j.n2));
    }
    *taken = eligible;
    if (!eligible) return AFV_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Blob b(c);
    const int nsets = 2 * njobs;
    const size_t desc_off = b.reserve((size_t)nsets * cap * 32);
    const size_t n_off = b.reserve((size_t)nsets * 4);
    const size_t pa_off = b.reserve((size_t)njobs * 4), pb_off = b.reserve((size_t)njobs * 4);
    bool any_ori = false;
    for (int i = 0; i < njobs; ++i) any_ori = any_ori || jobs[i].check_orientation;
    const size_t ang_off = any_ori ? b.reserve((size_t)nsets * cap * sizeof(float)) : 0;
    for (int i = 0; i < njobs; ++i) {
        const afv_match_job &j = jobs[i];
        if (j.n1) std::memcpy(b.h.data() + desc_off + (size_t)(2 * i) * cap * 32, j.desc1, (size_t)j.n1 * 32);
        if (j.n2) std::memcpy(b.h.data() + desc_off + (size_t)(2 * i + 1) * cap * 32, j.desc2, (size_t)j.n2 * 32);
        int32_t *n = reinterpret_cast<int32_t *>(b.h.data() + n_off);
        n[2 * i] = j.n1;
        n[2 * i + 1] = j.n2;
        reinterpret_cast<int32_t *>(b.h.data() + pa_off)[i] = 2 * i;
        reinterpret_cast<int32_t *>(b.h.data() + pb_off)[i] = 2 * i + 1;
        if (any_ori && j.check_orientation) {
            float *a1 = reinterpret_cast<float *>(b.h.data() + ang_off) + (size_t)(2 * i) * cap;
            std::memcpy(a1, j.angle1, (size_t)j.n1 * sizeof(float));
            std::memcpy(a1 + cap, j.angle2, (size_t)j.n2 * sizeof(float));
        }
    }
    const size_t match_off = b.reserve((size_t)njobs * cap * 4), nm_off = b.reserve((size_t)njobs * 4);
    const int nslices = small_batch_path(c, njobs) ? afv_match_topk_slices(cap, c->match_engine, ((cap + 63) / 64 + 1) / 2) : 1;
    const size_t topk_off = b.reserve_scratch((size_t)njobs * cap * 32);
    {
        const int rc_ = ensure_slice_scratch(c, njobs, cap, nslices);
        if (rc_) return rc_;
    }
    int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_match, b.h.data(), match_off, hipMemcpyHostToDevice, c->stream));  // inputs only
    // jobs may differ in mbCheckOrientation / thresholds: launch runs of identical settings
    int i0 = 0;
    while (i0 < njobs) {
        int i1 = i0 + 1;
        while (i1 < njobs && jobs[i1].th_low == jobs[i0].th_low && jobs[i1].nnratio == jobs[i0].nnratio &&
               (jobs[i1].check_orientation != 0) == (jobs[i0].check_orientation != 0))
            ++i1;
        const float *angp = any_ori ? reinterpret_cast<const float *>(c->d_match + ang_off) : nullptr;
        const int *np_ = reinterpret_cast<const int *>(c->d_match + n_off);
        const int *pa_ = reinterpret_cast<const int *>(c->d_match + pa_off), *pb_ = reinterpret_cast<const int *>(c->d_match + pb_off);
        afv_launch_match_topk(c->d_match + desc_off, np_, cap, pa_, pb_, i1 - i0, c->d_match + topk_off, i0, c->match_engine, nslices, c->d_slice, c->d_tickets, 8, c->stream);
        afv_launch_match_resolve(c->d_match + desc_off, angp, 1, np_, cap, pa_, pb_, i1 - i0, jobs[i0].th_low, jobs[i0].nnratio,
                                 jobs[i0].check_orientation != 0, reinterpret_cast<int *>(c->d_match + match_off),
                                 reinterpret_cast<int *>(c->d_match + nm_off), c->d_match + topk_off, i0, resolve_engine_for(c, njobs), 8, c->stream);
        i0 = i1;
    }
    HIPCHK(c, hipGetLastError());
    size_t acc = 0;
    for (int i = 0; i < njobs; ++i) {
        HIPCHK(c, b.fetch(out + acc, match_off + (size_t)i * cap * 4, (size_t)jobs[i].n1 * 4, c->stream));
        acc += (size_t)jobs[i].n1;
    }
    HIPCHK(c, b.fetch(nmatches, nm_off, (size_t)njobs * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.finish();
    return afv_check_resolve_guard(c, nmatches, njobs);
}

// afv_stereo.hip — host side of the stereo / RGB-D members of the device-resident Frame (include/afv_hip.h, "stereo and RGB-D frames";
// kernels: k_stereo.hip).
//
// Reference: Frame::ComputeStereoMatches (src/Frame.cc:465-645) reads both eyes' keypoints, descriptors and mvImagePyramid;
// Frame::ComputeStereoFromRGBD (:648-669) the depth image.  Here both eyes are resident frames of one context, and the pyramid levels stay
// with the frame that asked for them (afv_frame_params.keep_pyramid) or are handed over (afv_frame_set_pyramid), so mvuRight / mvDepth are
// made where the projection searches and the keyframe table read them.
#include "afv_runtime.h"

// level sizes of the context's pyramid for a w x h image (afv_build_geometry's own arithmetic)
static int stereo_level_sizes(afv_ctx *c, int w, int h, int *nlevels, int *lw, int *lh) {
    if (w < 1 || h < 1 || w > c->p.max_width || h > c->p.max_height) return AFV_EINVAL;
    Geo g;
    const int rc = afv_build_geometry(c->p, w, h, 1, g);
    if (rc) return rc;
    *nlevels = g.nlevels;
    for (int l = 0; l < g.nlevels; ++l) {
        lw[l] = g.lv[l].w;
        lh[l] = g.lv[l].h;
    }
    return AFV_OK;
}

extern "C" int afv_pyramid_level_sizes(afv_ctx *c, int width, int height, int32_t *nlevels, int32_t *lw, int32_t *lh) {
    if (!c || !nlevels || !lw || !lh) return AFV_EINVAL;
    int nl = 0, w[AFV_MAX_LEVELS], h[AFV_MAX_LEVELS];
    const int rc = stereo_level_sizes(c, width, height, &nl, w, h);
    if (rc) return AFV_EINVAL;
    *nlevels = nl;
    for (int l = 0; l < nl; ++l) {
        lw[l] = w[l];
        lh[l] = h[l];
    }
    return AFV_OK;
}

// the frame's own level storage for these sizes (allocated on first use, again when the geometry changes)
static int stereo_ensure_pyramid(afv_frame *f, int nlevels, const int *lw, const int *lh) {
    afv_ctx *c = f->c;
    bool same = f->d_pyr && f->pyr_levels == nlevels;
    for (int l = 0; same && l < nlevels; ++l) same = f->pyr_w[l] == lw[l] && f->pyr_h[l] == lh[l];
    if (same) return AFV_OK;
    size_t off = 0;
    size_t offs[AFV_MAX_LEVELS]{};
    for (int l = 0; l < nlevels; ++l) {
        offs[l] = off;
        off = align_up(off + (size_t)lw[l] * lh[l], 256);
    }
    f->has_pyramid = false;
    if (off > f->pyr_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (an earlier search may still read the old levels)
        if (f->d_pyr) (void)hipFree(f->d_pyr);
        f->d_pyr = nullptr;
        f->pyr_bytes = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&f->d_pyr), off));
        f->pyr_bytes = off;
    }
    f->pyr_levels = nlevels;
    for (int l = 0; l < nlevels; ++l) {
        f->pyr_w[l] = lw[l];
        f->pyr_h[l] = lh[l];
        f->pyr_off[l] = offs[l];
    }
    return AFV_OK;
}

int afv_frame_keep_pyramid(afv_frame *f, const FrameSrc &src, hipStream_t s) {
    afv_ctx *c = f->c;
    const Geo &g = c->geo;
    int lw[AFV_MAX_LEVELS], lh[AFV_MAX_LEVELS];
    for (int l = 0; l < g.nlevels; ++l) {
        lw[l] = g.lv[l].w;
        lh[l] = g.lv[l].h;
    }
    const int rc = stereo_ensure_pyramid(f, g.nlevels, lw, lh);
    if (rc) return rc;
    for (int l = 0; l < g.nlevels; ++l) {  // level 0 is the staged image, the others lie in the context's pyramid buffer (frame slot 0)
        const LevelGeo &L = g.lv[l];
        const uint8_t *sp = l == 0 ? src.base : c->d_pyr + L.pyr_off;
        const size_t spitch = l == 0 ? (size_t)src.stride : (size_t)L.pitch;
        HIPCHK(c, hipMemcpy2DAsync(f->d_pyr + f->pyr_off[l], (size_t)L.w, sp, spitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToDevice, s));
    }
    f->has_pyramid = true;
    return AFV_OK;
}

extern "C" int afv_frame_set_pyramid(afv_frame *f, int width, int height, const uint8_t *const *levels, int nlevels) {
    if (!f || !levels || nlevels < 1 || nlevels > AFV_MAX_LEVELS) return AFV_EINVAL;
    afv_ctx *c = f->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        int nl = 0, lw[AFV_MAX_LEVELS], lh[AFV_MAX_LEVELS];
        const int rc = stereo_level_sizes(c, width, height, &nl, lw, lh);
        if (rc) return rc == AFV_EUNSUPPORTED ? AFV_EINVAL : rc;
        if (nl != nlevels) return AFV_EINVAL;
        for (int l = 0; l < nl; ++l)
            if (!levels[l]) return AFV_EINVAL;
        const int rc2 = stereo_ensure_pyramid(f, nl, lw, lh);
        if (rc2) return rc2;
        hipStream_t s = c->stream;
        HIPCHK(c, hipStreamSynchronize(s));  // the arena below is the context's: nothing of an earlier call may still be reading it
        HostImage arena{c};
        arena.resize(f->pyr_off[nl - 1] + (size_t)lw[nl - 1] * lh[nl - 1], false);
        for (int l = 0; l < nl; ++l) std::memcpy(arena.data() + f->pyr_off[l], levels[l], (size_t)lw[l] * lh[l]);
        HIPCHK(c, hipMemcpyAsync(f->d_pyr, arena.data(), arena.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));
        f->has_pyramid = true;
        return AFV_OK;
    });
}

extern "C" int afv_frame_get_pyramid_level(afv_frame *f, int level, uint8_t *out) {
    if (!f || !out || !f->has_pyramid || level < 0 || level >= f->pyr_levels) return AFV_EINVAL;
    afv_ctx *c = f->c;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, f->d_pyr + f->pyr_off[level], (size_t)f->pyr_w[level] * f->pyr_h[level], hipMemcpyDeviceToHost));
    return AFV_OK;
}

extern "C" int afv_frame_stereo_match(afv_frame *left, afv_frame *right, const afv_stereo_params *params, int32_t *n_stereo) {
    if (!left || !right || !params) return AFV_EINVAL;
    if (params->struct_size < offsetof(afv_stereo_params, th_low) + sizeof(float) || params->struct_size > 4 * sizeof(afv_stereo_params)) return AFV_EINVAL;
    if (left->c != right->c) return AFV_EINVAL;  // frames of two contexts
    afv_ctx *c = left->c;
    if (!left->has_features || !right->has_features || !left->has_pyramid || !right->has_pyramid) {
        c->last_error = "afv_frame_stereo_match: both frames need features and a pyramid (keep_pyramid / afv_frame_set_pyramid)";
        return AFV_EINVAL;
    }
    if (left->float_dim != right->float_dim || left->desc_bytes != right->desc_bytes || left->words != right->words) return AFV_EUNSUPPORTED;
    if (left->pyr_levels != right->pyr_levels) return AFV_EUNSUPPORTED;
    for (int l = 0; l < left->pyr_levels; ++l)
        if (left->pyr_w[l] != right->pyr_w[l] || left->pyr_h[l] != right->pyr_h[l]) return AFV_EUNSUPPORTED;
    afv_stereo_params p{};
    std::memcpy(&p, params, std::min<size_t>(params->struct_size, sizeof(p)));
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t s = c->stream;
        DevStereoJob J{};
        J.kps_l = left->d_kps; J.kps_r = right->d_kps;
        J.size_l = left->d_size; J.size_r = right->d_size;
        J.desc_l = reinterpret_cast<const uint32_t *>(left->d_desc); J.desc_r = reinterpret_cast<const uint32_t *>(right->d_desc);
        J.n_l = left->n; J.n_r = right->n;
        J.words = left->words; J.fdim = left->float_dim;
        J.th_high = p.th_high;
        J.th_orb = (p.th_high + p.th_low) / 2.0f;  // :473
        J.mbf = p.mbf;
        const float mb = p.mbf / p.fx;              // Frame.cc:213
        J.max_d = p.mbf / mb;                       // :503 maxD = mbf / minZ, minZ = mb
        J.n_rows = left->pyr_h[0];                  // :475
        J.nlevels = left->pyr_levels;
        for (int l = 0; l < J.nlevels; ++l) {
            J.lw[l] = left->pyr_w[l];
            J.lh[l] = left->pyr_h[l];
            J.pyr_l[l] = left->d_pyr + left->pyr_off[l];
            J.pyr_r[l] = right->d_pyr + right->pyr_off[l];
        }
        J.u_right = left->d_ur; J.depth = left->d_depth; J.sad = left->d_sad; J.best_r = left->d_best_r; J.n_stereo = left->d_nstereo;
        left->has_depth = false;
        left->has_stereo = false;
        afv_launch_stereo_match(&J, s);
        afv_launch_stereo_median(J.u_right, J.depth, J.sad, J.n_l, J.n_stereo, s);
        HIPCHK(c, hipGetLastError());
        HostImage arena{c};
        arena.resize(256, false);
        int *h_n = reinterpret_cast<int *>(arena.data());
        HIPCHK(c, hipMemcpyAsync(h_n, J.n_stereo, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (*h_n < 0 || *h_n > left->n) return AFV_EHIP;
        left->has_depth = true;
        left->has_stereo = true;
        if (n_stereo) *n_stereo = *h_n;
        return AFV_OK;
    });
}

extern "C" int afv_frame_set_depth(afv_frame *f, const float *depth, int width, int height, int stride_bytes, float mbf) {
    if (!f || !depth || width < 1 || height < 1 || stride_bytes < 4 * width || (stride_bytes & 3)) return AFV_EINVAL;
    if (!f->has_features || (f->p.distorted && !f->has_grid)) return AFV_EINVAL;  // mvKeysUn.x of a distorted frame comes with afv_frame_set_undistorted
    afv_ctx *c = f->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t s = c->stream;
        HIPCHK(c, hipStreamSynchronize(s));  // the arena and the staging buffer are the context's
        const size_t row = (size_t)width * 4, bytes = row * (size_t)height;
        HostImage arena{c};
        arena.resize(bytes, false);
        for (int y = 0; y < height; ++y) std::memcpy(arena.data() + (size_t)y * row, reinterpret_cast<const uint8_t *>(depth) + (size_t)y * stride_bytes, row);
        const int rc = ensure_match_buffer(c, bytes);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_match, arena.data(), bytes, hipMemcpyHostToDevice, s));  // the image travels once per call
        f->has_depth = false;
        f->has_stereo = false;
        afv_launch_stereo_rgbd(f->d_kps, f->d_x, f->n, reinterpret_cast<const float *>(c->d_match), width, height, mbf, f->d_ur, f->d_depth, s);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(s));
        f->has_depth = true;
        return AFV_OK;
    });
}

extern "C" int afv_frame_get_stereo(afv_frame *f, float *u_right, float *depth, int32_t *sad, int32_t *best_r) {
    if (!f || !f->has_features) return AFV_EINVAL;
    afv_ctx *c = f->c;
    const size_t n = (size_t)f->n;
    if (!n) return AFV_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (u_right) HIPCHK(c, hipMemcpy(u_right, f->d_ur, n * 4, hipMemcpyDeviceToHost));
    if (depth) {
        if (f->has_depth) HIPCHK(c, hipMemcpy(depth, f->d_depth, n * 4, hipMemcpyDeviceToHost));
        else std::fill(depth, depth + n, -1.0f);  // mvDepth of a frame nobody gave depth to
    }
    if (sad) {
        if (f->has_stereo) HIPCHK(c, hipMemcpy(sad, f->d_sad, n * 4, hipMemcpyDeviceToHost));
        else std::fill(sad, sad + n, -1);
    }
    if (best_r) {
        if (f->has_stereo) HIPCHK(c, hipMemcpy(best_r, f->d_best_r, n * 4, hipMemcpyDeviceToHost));
        else std::fill(best_r, best_r + n, -1);
    }
    return AFV_OK;
}

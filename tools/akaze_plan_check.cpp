// akaze_plan_check.cpp — stand-alone host check of csrc/akaze_plan.hip (the pure host mathematics of the AKAZE61 path) under
// AddressSanitizer and UndefinedBehaviorSanitizer.  No device and no HIP call: it runs on any CPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -x c++ anyfeature-vslam_amd/csrc/akaze_plan.hip tools/akaze_plan_check.cpp -o tools/akaze_plan_check && tools/akaze_plan_check
// For 80 x 40 (the smallest frame), 83 x 40 (odd), 1280 x 720 (config #5) and 2048 x 1536 (the widest detection takes): the evolution plan,
// the detection layout (offsets monotone, sums equal to the strides, every grid inside its limits), the pinned arena.  And the level
// quotas of afv_level_quotas against written-out values of the recurrence.
#include <cstdio>
#include <cstring>

#include "../anyfeature-vslam_amd/csrc/akaze_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAILED %s: ", #cond);               \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++failures;                                      \
        }                                                    \
    } while (0)

static void check_size(int w, int h) {
    afv_akaze_params prm;
    afv_akaze_default_params(&prm);
    afv_akaze_plan P;
    const int rc = afv_akaze_plan_for(&prm, w, h, &P);
    CHECK(rc == AFV_OK, "%d x %d: plan rc %d", w, h, rc);
    if (rc) return;
    CHECK(P.nlevels >= prm.nsublevels && P.nlevels <= AFV_AKZ_MAX_LEVELS && P.w == w && P.h == h, "%d x %d: %d levels", w, h, P.nlevels);
    for (int i = 0; i < P.nlevels; ++i) {
        const afv_akaze_level &L = P.lv[i];
        CHECK(L.w == (w >> L.octave) && L.h == (h >> L.octave), "%d x %d level %d: %d x %d", w, h, i, L.w, L.h);
        CHECK(L.nsteps >= 0 && L.nsteps <= AFV_AKZ_MAX_FED && L.sigma_size >= 2 && L.sigma_size <= 8, "%d x %d level %d", w, h, i);
        float sum = 0;
        for (int k = 0; k < L.nsteps; ++k) sum += L.tau[k];
        if (i) CHECK(std::fabs(sum - (L.etime - P.lv[i - 1].etime)) < 1e-4f, "%d x %d level %d: FED steps add up to %g", w, h, i, sum);
    }
    AkdParams D;
    std::memset(&D, 0, sizeof D);
    const int grc = akz_detect_layout(P, prm.derivative_factor, D);
    CHECK(grc == AFV_OK, "%d x %d: layout rc %d", w, h, grc);
    int coff = 0, roff = 0, cells = 0, elems = 0, lds = 0, prev = 0;
    for (int i = 0; i < P.nlevels; ++i) {
        const AkdLevel &L = D.lv[i];
        CHECK(L.w == P.lv[i].w && L.h == P.lv[i].h && L.octave == P.lv[i].octave, "%d x %d level %d", w, h, i);
        CHECK(L.cand_off == coff && L.row_off == roff && L.cand_cap == L.w * L.h / 8 + 64, "%d x %d level %d: cand_off %d row_off %d cand_cap %d", w, h,
              i, L.cand_off, L.row_off, L.cand_cap);
        coff += L.cand_cap;
        roff += L.h;
        if (grc) continue;
        CHECK(L.gcell_off == cells && L.gelem_off == elems, "%d x %d level %d: gcell_off %d gelem_off %d", w, h, i, L.gcell_off, L.gelem_off);
        CHECK(L.gw >= 1 && L.gh >= 1 && L.gcap >= 1 && L.gcap <= 255 && L.ginv > 0, "%d x %d level %d: grid %d x %d cap %d", w, h, i, L.gw, L.gh, L.gcap);
        // a cell edge covers the search disc of this level and of the next one twice over
        CHECK(1.0f / L.ginv >= 2.0f * L.psize && (i + 1 == P.nlevels || 1.0f / L.ginv >= 2.0f * P.lv[i + 1].esigma * prm.derivative_factor),
              "%d x %d level %d: cell edge %g", w, h, i, 1.0f / L.ginv);
        const int nc = L.gw * L.gh;
        lds = std::max(lds, (nc + 15) / 16 * 16 + (prev + 15) / 16 * 16);
        prev = nc;
        cells += nc;
        elems += nc * L.gcap;
    }
    CHECK(D.cand_stride == coff && D.rows_stride == roff, "%d x %d: strides %d %d, sums %d %d", w, h, D.cand_stride, D.rows_stride, coff, roff);
    if (!grc) CHECK(D.gcells == cells && D.gelems == elems && D.lds_bytes == lds, "%d x %d: grids %d %d %d", w, h, D.gcells, D.gelems, D.lds_bytes);
    CHECK(D.nlevels == P.nlevels && D.W == w && D.H == h, "%d x %d", w, h);
    for (int nf = 1; nf <= 3; ++nf) {
        const size_t img = (size_t)w * h, oc = 1024;
        const AkzArena A(nf, img, oc);
        CHECK(A.in_bytes == nf * img && A.off_status >= A.in_bytes && A.off_count >= A.off_status + sizeof(int) &&
                  A.off_kps >= A.off_count + nf * sizeof(int) && A.off_desc >= A.off_kps + nf * oc * sizeof(afv_keypoint) &&
                  A.total == A.off_desc + nf * oc * 64,
              "%d x %d: arena of %d frames", w, h, nf);
        CHECK(A.off_status % 256 == 0 && A.off_count % 256 == 0 && A.off_kps % 256 == 0 && A.off_desc % 256 == 0, "%d x %d: arena alignment", w, h);
    }
    std::printf("%4d x %4d: %d levels, %d candidates, %d rows, %d cells, %d list elements, %d bytes of LDS per frame\n", w, h, P.nlevels, D.cand_stride,
                D.rows_stride, D.gcells, D.gelems, D.lds_bytes);
}

static void check_quotas(int nfeatures, float scale_factor, int nlevels, const int *want) {
    int q[AFV_AKZ_MAX_LEVELS + 1];
    q[nlevels] = -12345;  // canary
    afv_level_quotas(nfeatures, 1.0f / scale_factor, nlevels, q);
    int sum = 0;
    for (int l = 0; l < nlevels; ++l) {
        CHECK(q[l] == want[l], "quota (%d, %g, %d) level %d: %d, want %d", nfeatures, scale_factor, nlevels, l, q[l], want[l]);
        sum += q[l];
    }
    CHECK(sum == nfeatures && q[nlevels] == -12345, "quota (%d, %g, %d): sum %d", nfeatures, scale_factor, nlevels, sum);
}

int main() {
    const int sizes[4][2] = {{80, 40}, {83, 40}, {1280, 720}, {2048, 1536}};
    for (const auto &s : sizes) check_size(s[0], s[1]);
    // float desired = N (1 - f) / (1 - f^n), f = 1 / scaleFactor; level l takes round(desired), desired *= f; the last level takes the rest
    const int q1[8] = {217, 181, 151, 126, 105, 87, 73, 60}, q2[8] = {65, 54, 45, 38, 31, 26, 22, 19}, q3[6] = {146, 112, 86, 66, 51, 39},
              q4[8] = {212, 178, 150, 126, 106, 89, 75, 64};
    check_quotas(1000, 1.2f, 8, q1);
    check_quotas(300, 1.2f, 8, q2);
    check_quotas(500, 1.3f, 6, q3);
    check_quotas(1000, 1.1892f, 8, q4);
    afv_akaze_params prm;
    afv_akaze_default_params(&prm);
    int quota[AFV_AKZ_MAX_LEVELS] = {}, sel_cap = 0, out_cap = 0, M = 0;
    akz_quota_plan(prm, 8, quota, &sel_cap, &out_cap, &M);
    CHECK(std::memcmp(quota, q4, sizeof q4) == 0 && sel_cap == 212 + 3 && out_cap == 1000 + 3 * 8 && M == 256, "budget: %d %d %d", sel_cap, out_cap, M);
    std::printf(failures ? "akaze_plan_check: %d FAILED\n" : "akaze_plan_check ok\n", failures);
    return failures ? 1 : 0;
}

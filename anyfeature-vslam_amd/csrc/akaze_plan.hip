// akaze_plan.hip — the pure host mathematics of the AKAZE61 path: FED time steps, Gaussian taps, the evolution plan of an image size
// (afv_akaze_plan_for), the layout of a frame's detection arrays with the grids of the ordered suppression, the quadtree budget.
// No HIP call and no device state: akaze_api.hip drives the device with what this file computes.
#include <cstring>

#include "akaze_plan.h"

static inline int f_round(float x) { return (int)(x + 0.5f); }

// ---- FED time steps (libAKAZE fed.cpp) ----
static bool fed_is_prime(int n) {
    if (n <= 1) return false;
    if (n == 2 || n == 3 || n == 5 || n == 7) return true;
    if (n % 2 == 0 || n % 3 == 0 || n % 5 == 0 || n % 7 == 0) return false;
    const int upper = (int)(std::sqrt((double)n + 1.0));
    for (int d = 11; d <= upper; d += 2)
        if (n % d == 0) return false;
    return true;
}
static int fed_tau(float T, float tau_max, float *tau) {
    const int n = (int)(ceilf(sqrtf(3.0f * T / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
    if (n > AFV_AKZ_MAX_FED) return -1;
    if (n <= 0) return 0;
    const float scale = 3.0f * T / (tau_max * (float)(n * (n + 1)));
    float tauh[AFV_AKZ_MAX_FED];
    const float c = 1.0f / (4.0f * (float)n + 2.0f), d = scale * tau_max / 2.0f;
    for (int k = 0; k < n; ++k) {
        const float hcos = cosf(3.14159265358979323846f * (2.0f * (float)k + 1.0f) * c);
        tauh[k] = d / (hcos * hcos);
    }
    const int kappa = n / 2;
    int prime = n + 1;
    while (!fed_is_prime(prime)) prime++;
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return n;
}
static int gauss_ksize(float sigma) {
    int ks = (int)ceilf(2.0f * (1.0f + (sigma - 0.8f) / 0.3f));
    if ((ks % 2) == 0) ks += 1;
    return ks;
}
static void gauss_taps(float sigma, int n, float *k) {  // cv::getGaussianKernel(n, sigma, CV_32F), sigma > 0
    const double s = (double)sigma, scale2x = -0.5 / (s * s);
    double t[64], sum = 0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        t[i] = std::exp(scale2x * x * x);
        sum += t[i];
    }
    for (int i = 0; i < n; ++i) k[i] = (float)(t[i] / sum);
}

extern "C" void afv_akaze_default_params(afv_akaze_params *p) {
    if (!p) return;
    p->omax = 2; p->nsublevels = 4; p->soffset = 1.6f; p->derivative_factor = 1.5f;
    p->dthreshold = 0.0005f; p->min_dthreshold = 0.00001f; p->kcontrast_percentile = 0.7f; p->kcontrast_nbins = 300;
    p->max_width = 1280; p->max_height = 720; p->max_batch = 1;
    p->nfeatures = 1000; p->scale_factor = 1.1892f;  // Tracking.cc:1515-1520, settings/akaze61_settings.yaml:7
}

extern "C" int afv_akaze_plan_for(const afv_akaze_params *o, int w, int h, afv_akaze_plan *p) {
    if (!o || !p || w < 16 || h < 16 || o->omax < 1 || o->nsublevels < 1) return AFV_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->w = w; p->h = h;
    int n = 0;
    for (int i = 0; i < o->omax; ++i) {
        const float rfactor = 1.0f / powf(2.0f, (float)i);
        const int lh = (int)((float)h * rfactor), lw = (int)((float)w * rfactor);
        if ((lw < 80 || lh < 40) && i != 0) break;
        for (int j = 0; j < o->nsublevels; ++j) {
            if (n >= AFV_AKZ_MAX_LEVELS) return AFV_EINVAL;
            afv_akaze_level &L = p->lv[n++];
            L.w = lw; L.h = lh; L.octave = i; L.sublevel = j;
            L.esigma = o->soffset * powf(2.0f, (float)j / (float)o->nsublevels + (float)i);
            L.etime = 0.5f * (L.esigma * L.esigma);
            L.sigma_size = f_round(L.esigma * o->derivative_factor / powf(2.0f, (float)i));
            if (L.sigma_size < 2 || L.sigma_size > 8) return AFV_EUNSUPPORTED;  // sparse-tap Scharr path (k_akz_deriv1)
        }
    }
    p->nlevels = n;
    for (int i = 1; i < n; ++i) {
        const int ns = fed_tau(p->lv[i].etime - p->lv[i - 1].etime, 0.25f, p->lv[i].tau);
        if (ns < 0) return AFV_EUNSUPPORTED;
        p->lv[i].nsteps = ns;
        if (p->lv[i].octave > p->lv[i - 1].octave && ((p->lv[i - 1].w & 1) || (p->lv[i - 1].h & 1))) return AFV_EUNSUPPORTED;  // exact 2x INTER_AREA only
    }
    p->ksize_soffset = gauss_ksize(o->soffset);
    p->ksize_one = gauss_ksize(1.0f);
    if (p->ksize_soffset > 13 || p->ksize_one > 7) return AFV_EUNSUPPORTED;
    gauss_taps(o->soffset, p->ksize_soffset, p->gauss_soffset);
    gauss_taps(1.0f, p->ksize_one, p->gauss_one);
    return AFV_OK;
}

// Grids of the ordered suppression (k_akaze_detect.hip, AkdLevel): level c's entries are searched with the radii of levels c-1
// (upper-level filter), c and c+1, so its cell edge is twice the largest of those (a disc then overlaps at most 2 x 2 cells);
// a list can never hold more elements than there are strict 3 x 3 maxima of level c inside one cell.
static int akz_grid_geometry(const afv_akaze_plan &P, float derivative_factor, AkdLevel *lv, int *gcells, int *gelems, int *lds_bytes) {
    int cells = 0, elems = 0, lds = 0, prev_cells = 0;
    for (int i = 0; i < P.nlevels; ++i) {
        const float r = P.lv[i].esigma * derivative_factor;
        const float rn = i + 1 < P.nlevels ? P.lv[i + 1].esigma * derivative_factor : r;
        const float edge = 2.0f * std::max(r, rn) * 1.0002f + 0.01f;
        const float ratio = powf(2.0f, (float)P.lv[i].octave);
        AkdLevel &L = lv[i];
        L.ginv = 1.0f / edge;
        L.gw = (int)((float)P.w * L.ginv) + 1;
        L.gh = (int)((float)P.h * L.ginv) + 1;
        const int side = (int)(edge / ratio) + 2;  // pixel positions of this level along one cell edge
        L.gcap = ((side + 1) / 2) * ((side + 1) / 2);
        if (L.gw >= 65536 || L.gh >= 16384 || L.gcap > 255) return AFV_EUNSUPPORTED;  // akd_box packing, u8 list lengths
        L.gcell_off = cells;
        L.gelem_off = elems;
        const int nc = L.gw * L.gh;
        lds = std::max(lds, ((nc + 15) & ~15) + ((prev_cells + 15) & ~15));
        prev_cells = nc;
        cells += nc;
        elems += nc * L.gcap;
    }
    *gcells = cells; *gelems = elems; *lds_bytes = lds;
    return AFV_OK;
}

int akz_detect_layout(const afv_akaze_plan &P, float derivative_factor, AkdParams &D) {
    D.nlevels = P.nlevels; D.W = P.w; D.H = P.h;
    int coff = 0, roff = 0;
    for (int i = 0; i < P.nlevels; ++i) {
        AkdLevel &L = D.lv[i];
        L.w = P.lv[i].w; L.h = P.lv[i].h; L.octave = P.lv[i].octave;
        L.psize = P.lv[i].esigma * derivative_factor;
        L.ratio = powf(2.0f, (float)P.lv[i].octave);
        L.sigma_size = (int)(L.psize / L.ratio + 0.5f);
        L.cand_off = coff; L.cand_cap = L.w * L.h / 8 + 64; L.row_off = roff;
        coff += L.cand_cap; roff += L.h;
    }
    D.cand_stride = coff; D.rows_stride = roff;
    return akz_grid_geometry(P, derivative_factor, D.lv, &D.gcells, &D.gelems, &D.lds_bytes);
}

void akz_quota_plan(const afv_akaze_params &prm, int nlevels, int *quota, int *sel_cap, int *out_cap, int *qt_M) {
    afv_level_quotas(prm.nfeatures, 1.0f / prm.scale_factor, nlevels, quota);
    const int qmax = *std::max_element(quota, quota + nlevels);
    *sel_cap = qmax + 3;
    *out_cap = prm.nfeatures + 3 * nlevels;
    *qt_M = (std::max(qmax + 8, 4 * 16 + 8) + 63) / 64 * 64;  // 16: the most quadtree roots a frame can have (n_ini, akz_describe_enqueue)
}

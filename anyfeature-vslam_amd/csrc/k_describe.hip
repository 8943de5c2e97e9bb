// k_describe.hip — E6 + E9 + E10 + E11 fused: IC angle, 7x7 Gaussian blur and rotated BRIEF, one wavefront
// per selected keypoint; plus the standalone level blur used by afv_debug_blur_level.
//
// Replaces ICAngles (cv::ORB::detect, Feature_orb32.cpp:34 == IC_Angle ORBextractor.cc:143-170), the
// GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) of every pyramid level and computeOrbDescriptors inside each
// cv::ORB::compute call (Feature_orb32.cpp:48; same arithmetic as computeOrbDescriptor FeatureExtractor.h:178-217),
// and mergeKeypointLevels (FeatureExtractor.cpp:296-308).
//
// The reference blurs whole levels (36 level-blurs per frame because compute() is called once per level).  Only the
// 512 rotated test locations inside the 37x37 neighbourhood of a keypoint are ever sampled, so each wavefront stages
// the 43x43 UNBLURRED patch around its keypoint in LDS (reflect-101 at the image edge = cv::ORB's apron), computes
// the intensity-centroid moments from it, runs the ROW pass of the blur over the patch once (integer taps
// [18,34,49,55,49,34,18], v_dot4_u32_u8 on the aligned dwords with the taps laid out per output, exact in 16 bits; the lane -> (row group,
// dword group) mapping is fixed, the loop unrolled, the loads of a step issued before the store of the step before) and evaluates the COLUMN
// pass + round-half-even(S/65536) only at the sampled locations.  The row-filtered plane is stored as INTERLEAVED ROW PAIRS (one dword =
// rows 2j and 2j + 1 of a column): the seven rows of a sample are four dwords at one address + immediates, four v_dot2_u32_u16
// (-DDS_ROW_MAJOR_PLANE keeps the u16 row-major plane of rounds 1-6 for A / B runs).  A test that falls outside the level ROI reads the
// unblurred apron pixel, as in OpenCV where only the ROI is blurred in place.  No blurred image ever touches HBM.
#include "afv_device.h"
#include "afv_wave.h"
#include "afv_runtime.h"  // the launchers below are declared there: a signature that drifts is a compile error, not a silent ABI mismatch

// the 256 test pairs (x0, y0, x1, y1) as floats (FeatureExtractor.h:219-477): one 16-byte load per test, no conversions
__device__ __constant__ __attribute__((aligned(16))) const float k_brief_pattern[1024] = {
#include "brief_pattern.inc"
};

// IC stage: lane = (row v = (lane >> 1) - 15, half): the four byte masks of the lane's 16-byte run (which bytes lie inside the disc) depend
// on the lane only - a table instead of ~24 vector instructions of min / max / shift per keypoint
struct IcMasks {
    uint32_t m[64][4];
};
constexpr IcMasks ic_make_masks() {
    IcMasks t{};
    // umax[v], v = 0..15: last column of row v of the radius-15 disc (orb.cpp / ORBextractor.cc:124-139)
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    for (int lane = 0; lane < 64; ++lane) {
        const int v = (lane >> 1) - 15, half = lane & 1;
        for (int q = 0; q < 4; ++q) {
            uint32_t m = 0;
            if (v <= 15) {
                const int d = umax[v < 0 ? -v : v];
                if (half) {
                    int nb = d + 1 - 4 * q;  // valid leading bytes
                    nb = nb < 0 ? 0 : (nb > 4 ? 4 : nb);
                    m = nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
                } else {
                    int nz = 16 - d - 4 * q;  // invalid leading bytes
                    nz = nz < 0 ? 0 : (nz > 4 ? 4 : nz);
                    m = nz >= 4 ? 0u : (0xffffffffu << (8 * nz));
                }
            }
            t.m[lane][q] = m;
        }
    }
    return t;
}
__device__ __constant__ __attribute__((aligned(16))) const IcMasks k_ic_masks = ic_make_masks();

#define PR 21        // patch radius: 18 (BRIEF reach) + 3 (blur)
#define PS 43        // patch side
#define PP 52        // LDS pitch of the patch rows: 13 dwords (odd => conflict-free row strides)
#define KP_PER_BLOCK AFV_KP_PER_BLOCK  // afv_device.h (the host plan of the block list divides by it too)

// cv::fastAtan2 (OpenCV mathfuncs_core atan_f32), degrees
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float rad2deg = (float)(180.0 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * rad2deg, p3 = -0.3258083974640975f * rad2deg;
    const float p5 = 0.1555786518463281f * rad2deg, p7 = -0.04432655554792128f * rad2deg;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + 2.2204460492503131e-16f);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + 2.2204460492503131e-16f);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// cos/sin of angle_deg*(pi/180) (float product, as FeatureExtractor.h:181): explicit double algorithm (Cody-Waite by
// pi/2 + Taylor), rounded once to float — bit-identical to the oracle's restatement, independent of any libm.
__device__ __forceinline__ void sincos_deg(float angle_deg, float &c_out, float &s_out) {
    const float factor_pi = (float)(3.1415926535897932384626433832795 / 180.f);
    const double t = (double)(angle_deg * factor_pi);
    const double kd = floor(t * 0.63661977236758138 + 0.5);
    const int k = (int)kd;
    const double r = (t - kd * 1.5707963267341256e+00) - kd * 6.0771005065061922e-11;
    const double z = r * r;
    const double sp = 1.0 + z * (-1.6666666666666666e-01 + z * (8.3333333333333332e-03 + z * (-1.9841269841269841e-04 +
                      z * (2.7557319223985893e-06 + z * (-2.5052108385441720e-08 + z * (1.6059043836821613e-10 +
                      z * (-7.6471637318198164e-13)))))));
    const double s = r * sp;
    const double c = 1.0 + z * (-0.5 + z * (4.1666666666666664e-02 + z * (-1.3888888888888889e-03 + z * (2.4801587301587302e-05 +
                     z * (-2.7557319223985888e-07 + z * (2.0876756987868100e-09 + z * (-1.1470745597729725e-11 +
                     z * (4.7794773323873853e-14))))))));
    double co, si;
    switch (k & 3) {
    case 0: co = c; si = s; break;
    case 1: co = -s; si = c; break;
    case 2: co = -c; si = -s; break;
    default: co = s; si = -c; break;
    }
    c_out = (float)co;
    s_out = (float)si;
}

// LDS hand-off between lanes of ONE wavefront: DS operations of a wave execute in order, so only the compiler has
// to be kept from moving the reads above the writes.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// round-half-even(S / 65536) saturated to 255.  S < 2^24 whenever the result is not saturated, so u32 -> f32 is exact, the scaling by
// 2^-16 is exact, and v_cvt_pk_u8_f32 rounds to nearest even and clamps: identical to the integer rule for every S the filter can
// produce (all 16 842 496 values checked on the device: tools/probes/probe_cvt_pk_u8.hip)
__device__ __forceinline__ uint32_t blur_round(uint32_t S) { return __builtin_amdgcn_cvt_pk_u8_f32((float)S * (1.0f / 65536.0f), 0, 0u); }

// Row pass of the separable 8U filter over the whole staged patch, once per keypoint: H[r][xh] = sum_k taps[k] * P[r][xh + k]
// for xh = 0..39 (<= 257 * 255 = 65535: exact in 16 bits).  One lane per group of 4 adjacent outputs: 3 aligned dwords in, ten
// v_dot4_u32_u8, 4 x u16 out.
#ifndef HP
#define HP 40  // u16 pitch of a plane row (80 bytes: 8-byte aligned rows, no padding: 44 cost a workgroup of occupancy per CU)
#endif
#define ROW_GROUPS 10                 // dword groups of a plane row (HP / 4)
#define ROW_LANES 6                   // (pair-)rows per wave step: lane = (lane / 10, lane % 10), lanes 60..63 idle
#define GP (4 * HP)                   // interleaved plane: bytes of a pair-row (HP dwords)
#define PAIR_ROWS ((PS + 1) / 2)      // 22: pair-row 21 = (row 42, 0)
static_assert(HP == 4 * ROW_GROUPS && ROW_GROUPS * ROW_LANES <= 64, "row pass: lane mapping");
static_assert(4 * (ROW_GROUPS - 1) + 12 <= PP, "row pass: the three dwords of the last group lie inside the patch row");

// the four outputs of a group: output k = taps over bytes k .. k + 6 of the 12-byte window (d0, d1, d2).  Instead of shifting the DATA to the taps
// (two funnel shifts per output) the TAPS are laid out at the byte positions of every k - constants in scalar registers,
// 2 + 2 + 3 + 3 dot products and no shifts
__device__ __forceinline__ void row_taps4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t (&o)[4]) {
    constexpr unsigned long long TAPS = 18ull | (34ull << 8) | (49ull << 16) | (55ull << 24) | (49ull << 32) | (34ull << 40) | (18ull << 48);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the 7 taps shifted up by k bytes inside a 96-bit field: its three dwords
        const unsigned __int128 F = (unsigned __int128)TAPS << (8 * k);
        const uint32_t t0 = (uint32_t)F, t1 = (uint32_t)(F >> 32), t2 = (uint32_t)(F >> 64);
        uint32_t a = __builtin_amdgcn_udot4(d1, t1, __builtin_amdgcn_udot4(d0, t0, 0u, false), false);
        if (t2) a = __builtin_amdgcn_udot4(d2, t2, a, false);
        o[k] = a;
    }
}

typedef unsigned short ushort2d __attribute__((ext_vector_type(2)));

// (a & 0xffffff) * b + c with b a wave-uniform 24-bit constant, as ONE v_mad_u32_u24: written as a + b * ... in C the compiler re-associates
// the sum with the shift-add that feeds it and ends up with a multiply, a shift and a three-input add
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

#ifdef DS_ROW_MAJOR_PLANE
// ---- u16 row-major plane (rounds 1-6; kept for A / B runs): H[r][xh] at u16 index r * HP + xh ----
#define PLANE_BYTES (PS * HP * 2)
#define ROW_STEPS ((PS + ROW_LANES - 1) / ROW_LANES)  // 8: rows rg, rg + 6, ..., rg + 42 (the last one for rg = 0 only)
__device__ __forceinline__ void blur_rows(const uint8_t *P, uint8_t *plane, int lane) {
    const uint32_t rg = ((uint32_t)lane * 205u) >> 11, g = (uint32_t)lane - rg * ROW_GROUPS;  // lane / 10, lane % 10 (lane < 64)
    if (lane >= ROW_GROUPS * ROW_LANES) return;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P + rg * PP + g * 4);
    uint2 *dst = reinterpret_cast<uint2 *>(plane + rg * (2 * HP) + g * 8);
    uint32_t d[3] = {src[0], src[1], src[2]}, n[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < ROW_STEPS; ++k) {
        const bool last = (k + 1) * ROW_LANES + ROW_LANES > PS;  // step k + 1 has rows past the patch
        // the loads of step k + 1 BEFORE the store of step k (the slice layout below: that store cannot reach them)
        if (k + 1 < ROW_STEPS && (!last || rg < PS - (k + 1) * ROW_LANES)) {
            const uint32_t *s = src + (k + 1) * ROW_LANES * (PP / 4);
            n[0] = s[0], n[1] = s[1], n[2] = s[2];
        }
        uint32_t o[4];
        row_taps4(d[0], d[1], d[2], o);
        uint2 w;
        w.x = o[0] | (o[1] << 16);
        w.y = o[2] | (o[3] << 16);
        if (k * ROW_LANES + ROW_LANES <= PS || rg < PS - k * ROW_LANES) dst[k * ROW_LANES * (2 * HP / 8)] = w;
        d[0] = n[0], d[1] = n[1], d[2] = n[2];
    }
}

// column pass + rounding with c = &H[yy][xh] (yy = y - 3, xh = x - 3: taps centred on patch position (x, y)): exact integer arithmetic
// of the separable filter, then round-half-even(S / 65536)
__device__ __forceinline__ int blur_col(const uint16_t *c) {
    // symmetric taps: rows k and 6 - k share a weight -> three v_dot2_u32_u16 on (row k, row 6 - k) pairs + the centre row
    ushort2d p0, p1, p2, t0, t1, t2;
    p0.x = c[0];
    p0.y = c[6 * HP];
    p1.x = c[HP];
    p1.y = c[5 * HP];
    p2.x = c[2 * HP];
    p2.y = c[4 * HP];
    t0.x = t0.y = 18;
    t1.x = t1.y = 34;
    t2.x = t2.y = 49;
    uint32_t S = 55u * (uint32_t)c[3 * HP];
    S = __builtin_amdgcn_udot2(p0, t0, S, false);
    S = __builtin_amdgcn_udot2(p1, t1, S, false);
    S = __builtin_amdgcn_udot2(p2, t2, S, false);
    return (int)blur_round(S);
}
__device__ __forceinline__ int blur_at(const uint8_t *plane, int x, int y) {
    // 24-bit multiply (y - 3 is 0 .. 36): a plain int product is a quarter-rate v_mul_lo_u32
    return blur_col(reinterpret_cast<const uint16_t *>(plane) + (__umul24((uint32_t)(y - 3), (uint32_t)HP) + (uint32_t)(x - 3)));
}
// interior sample straight from the float bits fx = 0x4B400000 + ix, fy = 0x4B400000 + iy (the rounding trick of the caller): byte address
// lds(plane) + 2 ((18 + iy) HP + 18 + a + ix) = 2 HP * (fy & 0xffffff) + 2 fx + k_addr (mod 2^32) - one shift-add, one 24-bit multiply-add
__device__ __forceinline__ uint32_t blur_addr_const(uint32_t lds_plane, int a) {
    return lds_plane + 2u * (uint32_t)((PR - 3) * HP + PR - 3 + a) - 2u * 0x4B400000u - (uint32_t)(2 * HP) * 0x400000u;
}
__device__ __forceinline__ int blur_bits(int fx, int fy, uint32_t k_addr) {
    const uint32_t addr = mad_u24((uint32_t)fy, (uint32_t)(2 * HP), ((uint32_t)fx << 1) + k_addr);
    return blur_col((const uint16_t *)(__attribute__((address_space(3))) const uint16_t *)(uintptr_t)addr);
}
#else
// ---- plane of interleaved row pairs: G[j][xh] = H[2j][xh] | H[2j + 1][xh] << 16, j = 0..21, one dword per column, pair-rows GP = 160 bytes
// apart; H[43] (no such patch row) = 0.  Item = (pair-row, dword group): two patch rows in, 20 dot products, 4 v_lshl_or, one 16-byte store ----
#define PLANE_BYTES (PAIR_ROWS * GP)
#define ROW_STEPS ((PAIR_ROWS + ROW_LANES - 1) / ROW_LANES)  // 4: pair-rows jg, jg + 6, jg + 12, jg + 18 (the last one for jg < 4)
__device__ __forceinline__ void blur_rows(const uint8_t *P, uint8_t *plane, int lane) {
    const uint32_t jg = ((uint32_t)lane * 205u) >> 11, g = (uint32_t)lane - jg * ROW_GROUPS;  // lane / 10, lane % 10 (lane < 64)
    if (lane >= ROW_GROUPS * ROW_LANES) return;
    constexpr int LAST = (ROW_STEPS - 1) * ROW_LANES;        // first pair-row of the last step
    constexpr bool ODD_TAIL = (PS & 1) != 0;                 // the last pair-row has no upper row
    const uint32_t *src = reinterpret_cast<const uint32_t *>(P + jg * (2 * PP) + g * 4);
    uint4 *dst = reinterpret_cast<uint4 *>(plane + jg * GP + g * 16);
    uint32_t d[6] = {src[0], src[1], src[2], src[PP / 4], src[PP / 4 + 1], src[PP / 4 + 2]}, n[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < ROW_STEPS; ++k) {
        // the loads of step k + 1 BEFORE the store of step k (the slice layout below: that store cannot reach them).  Nothing past the
        // slice is read: pair-rows >= PAIR_ROWS are skipped and the missing upper row of the last pair-row stays 0
        if (k + 1 < ROW_STEPS) {
            const uint32_t *s = src + (k + 1) * ROW_LANES * (2 * PP / 4);
            const bool tail = k + 1 == ROW_STEPS - 1;
            if (!tail || jg < PAIR_ROWS - LAST) n[0] = s[0], n[1] = s[1], n[2] = s[2];
            if (!tail || jg < PAIR_ROWS - LAST - (ODD_TAIL ? 1 : 0)) n[3] = s[PP / 4], n[4] = s[PP / 4 + 1], n[5] = s[PP / 4 + 2];
        }
        uint32_t e[4], o[4];
        row_taps4(d[0], d[1], d[2], e);
        row_taps4(d[3], d[4], d[5], o);
        uint4 w;
        w.x = e[0] | (o[0] << 16);
        w.y = e[1] | (o[1] << 16);
        w.z = e[2] | (o[2] << 16);
        w.w = e[3] | (o[3] << 16);
        if (k < ROW_STEPS - 1 || jg < PAIR_ROWS - LAST) dst[k * ROW_LANES * (GP / 16)] = w;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = n[i], n[i] = 0u;
    }
}

// column pass + rounding with c = &G[yy >> 1][xh] and sh = 16 * (yy & 1) in its low five bits (yy = y - 3, xh = x - 3: taps centred on
// patch position (x, y)).  The seven rows yy .. yy + 6 are the u16 slots (yy & 1) .. (yy & 1) + 6 of the four dwords c[0], c[HP], c[2 HP],
// c[3 HP]: funnel-shifted down by the parity they meet the tap pairs (18, 34) (49, 55) (49, 34) (18, 0) - no permutes, no centre multiply.
// yy <= 36, so the last dword is pair-row <= 21; slot 7 (weight 0) is H[43] = 0 at most.  Exact integer arithmetic of the separable filter,
// then round-half-even(S / 65536)
__device__ __forceinline__ int blur_col(const uint32_t *c, uint32_t sh) {
    const uint32_t d0 = c[0], d1 = c[HP], d2 = c[2 * HP], d3 = c[3 * HP];
    const uint32_t e0 = __builtin_amdgcn_alignbit(d1, d0, sh), e1 = __builtin_amdgcn_alignbit(d2, d1, sh), e2 = __builtin_amdgcn_alignbit(d3, d2, sh),
                   e3 = d3 >> (sh & 31u);
    ushort2d t0, t1, t2, t3;
    t0.x = 18, t0.y = 34;
    t1.x = 49, t1.y = 55;
    t2.x = 49, t2.y = 34;
    t3.x = 18, t3.y = 0;
    uint32_t S = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2d, e0), t0, 0u, false);
    S = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2d, e1), t1, S, false);
    S = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2d, e2), t2, S, false);
    S = __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2d, e3), t3, S, false);
    return (int)blur_round(S);
}
__device__ __forceinline__ int blur_at(const uint8_t *plane, int x, int y) {
    const uint32_t yy = (uint32_t)(y - 3);  // 0 .. 36
    // 24-bit multiply: a plain int product is a quarter-rate v_mul_lo_u32
    return blur_col(reinterpret_cast<const uint32_t *>(plane) + (__umul24(yy >> 1, (uint32_t)HP) + (uint32_t)(x - 3)), yy << 4);
}
// interior sample straight from the float bits fx = 0x4B400000 + ix, fy = 0x4B400000 + iy (the rounding trick of the caller): with
// jb = (fy & 0xffffff) >> 1 = 0x200000 + (iy >> 1) (0x400000 and PR - 3 = 18 are even: the floor commutes) the byte address is
// lds(plane) + GP ((18 + iy) >> 1) + 4 (18 + a + ix) = GP * jb + 4 fx + k_addr (mod 2^32) - a bit-field extract, one shift-add, one 24-bit
// multiply-add; the parity of yy = 18 + iy is bit 0 of fy
static_assert(((PR - 3) & 1) == 0, "blur_bits: the parity of a plane row is the parity of iy");
__device__ __forceinline__ uint32_t blur_addr_const(uint32_t lds_plane, int a) {
    return lds_plane + (uint32_t)(GP * ((PR - 3) / 2) + 4 * (PR - 3 + a)) - 4u * 0x4B400000u - (uint32_t)GP * 0x200000u;
}
__device__ __forceinline__ int blur_bits(int fx, int fy, uint32_t k_addr) {
    const uint32_t jb = ((uint32_t)fy >> 1) & 0x7fffffu;
    const uint32_t addr = mad_u24(jb, (uint32_t)GP, ((uint32_t)fx << 2) + k_addr);
    return blur_col((const uint32_t *)(__attribute__((address_space(3))) const uint32_t *)(uintptr_t)addr, (uint32_t)fy << 4);
}
#endif

// ---- what a BRIEF test can reach: the corners of the 43 x 43 patch are never read, at any angle ----
// A pattern point at radius r lands, rotated and rounded, on a pixel whose unit square meets the circle of radius r: that ring bound is the
// reachable set R (tests/test_describe_reach_cpu.py sweeps the angle with the kernel's own fp32 products and finds exactly this set: 1124 of the
// 37 x 37 positions).  From R, all at compile time and from the pattern constants the kernel includes:
//   H values  = R dilated by the seven rows of the column pass (1347 of 43 x 40);
//   row items = (pair-row, dword group) of the FOUR dwords blur_col reads per sample (the eighth u16 has weight 0 but its item is computed all
//               the same: no sample dword is ever stale), per alignment a = px0 & 3: 189 or 190 of 220 - three wave steps instead of four;
//   patch     = the seven bytes under every H value and the IC disc of ic_make_masks, as aligned dwords per alignment: 425 .. 442 of 516 -
//               seven load / store steps of 64 lanes instead of nine of 60.
// The union over the four alignments fits neither budget (198 items, 460 dwords): one table per alignment, selected by a scalar.
#define RCH_R (PR - 3)                 // 18: BRIEF reach
#define RCH_SIDE (2 * RCH_R + 1)       // 37
#define RCH_ROW_STEPS 3
#define RCH_STAGE_STEPS 7
#define RCH_PAIR_ROWS ((PS + 1) / 2)
#define RCH_GP (4 * HP)                                  // bytes of a pair-row of the interleaved plane
#define RCH_P_OFF (RCH_PAIR_ROWS * RCH_GP - PS * PP)     // first patch byte of the slice
struct Reach {
    bool R[RCH_SIDE][RCH_SIDE];          // [iy + 18][ix + 18]
    int n_R, n_H;
    int n_items[4], n_dwords[4];
    uint16_t item[4][64 * RCH_ROW_STEPS];      // pair-row << 8 | dword group, sorted; padded with copies of the last one
    uint16_t dword[4][64 * RCH_STAGE_STEPS];   // patch row << 8 | dword of the row, sorted; padded with copies of the last one
    bool fits, covered, overlay_ok, tail_ok;
};
constexpr Reach reach_make() {
    Reach t{};
    constexpr signed char pat[1024] = {
#include "brief_pattern.inc"
    };
    // has[s]: a pattern point with x^2 + y^2 = s exists; cnt = prefix sums
    int cnt[2 * RCH_R * RCH_R + 2] = {};
    bool in_reach = true;
    for (int i = 0; i < 512; ++i) {
        const int s = pat[2 * i] * pat[2 * i] + pat[2 * i + 1] * pat[2 * i + 1];
        if (4 * s >= RCH_SIDE * RCH_SIDE) in_reach = false;  // radius >= 18.5 could round to 19
        else cnt[s + 1] = 1;
    }
    for (int s = 1; s < 2 * RCH_R * RCH_R + 2; ++s) cnt[s] += cnt[s - 1];  // cnt[s] = radii^2 below s
    // pixel (ix, iy): the squared distances of its unit square from the centre span [lo / 4, hi / 4]
    bool H[PS][RCH_SIDE] = {};
    for (int iy = -RCH_R; iy <= RCH_R; ++iy)
        for (int ix = -RCH_R; ix <= RCH_R; ++ix) {
            const int ax = ix < 0 ? -ix : ix, ay = iy < 0 ? -iy : iy;
            const int mx = ax ? 2 * ax - 1 : 0, my = ay ? 2 * ay - 1 : 0;
            const int lo = (mx * mx + my * my + 3) / 4;                          // smallest s with 4 s >= lo4
            int hi = ((2 * ax + 1) * (2 * ax + 1) + (2 * ay + 1) * (2 * ay + 1)) / 4;  // largest s with 4 s <= hi4
            if (hi > 2 * RCH_R * RCH_R) hi = 2 * RCH_R * RCH_R;
            if (lo <= hi && cnt[hi + 1] - cnt[lo] > 0) {
                t.R[iy + RCH_R][ix + RCH_R] = true;
                ++t.n_R;
                for (int k = 0; k < 7; ++k) H[iy + RCH_R + k][ix + RCH_R] = true;  // plane rows yy .. yy + 6, yy = 18 + iy
            }
        }
    for (int r = 0; r < PS; ++r)
        for (int c = 0; c < RCH_SIDE; ++c) t.n_H += H[r][c] ? 1 : 0;
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};  // the disc of ic_make_masks
    t.fits = in_reach;
    t.covered = t.overlay_ok = t.tail_ok = true;
    for (int a = 0; a < 4; ++a) {
        // row items: the four dwords of every reachable sample (plane column xh = 18 + a + ix)
        bool it[RCH_PAIR_ROWS][ROW_GROUPS] = {};
        for (int y = 0; y < RCH_SIDE; ++y)
            for (int x = 0; x < RCH_SIDE; ++x)
                if (t.R[y][x])
                    for (int d = 0; d < 4; ++d) {
                        const int j = (y >> 1) + d, g = (x + a) >> 2;
                        if (j >= RCH_PAIR_ROWS || g >= ROW_GROUPS) t.covered = false;
                        else it[j][g] = true;
                    }
        int n = 0;
        for (int j = 0; j < RCH_PAIR_ROWS; ++j)
            for (int g = 0; g < ROW_GROUPS; ++g)
                if (it[j][g]) {
                    if (n < 64 * RCH_ROW_STEPS) t.item[a][n] = (uint16_t)(j << 8 | g);
                    ++n;
                }
        t.n_items[a] = n;
        if (n > 64 * RCH_ROW_STEPS || n <= 64 * (RCH_ROW_STEPS - 1)) t.fits = false;
        for (int i = n; i < 64 * RCH_ROW_STEPS && n > 0; ++i) t.item[a][i] = t.item[a][n - 1];
        // the overlay: every plane byte stored in steps 0 .. k lies below the first patch byte loaded in step k + 1; the pair-row without an
        // upper patch row (the last one) is met in the last step only
        int store_end = 0;
        for (int k = 0; k < RCH_ROW_STEPS; ++k) {
            int load_lo = 1 << 30;
            for (int i = 64 * k; i < 64 * k + 64; ++i) {
                const int j = t.item[a][i] >> 8, g = t.item[a][i] & 255;
                const int src = RCH_P_OFF + 2 * j * PP + 4 * g;
                load_lo = src < load_lo ? src : load_lo;
                if (j == RCH_PAIR_ROWS - 1 && k != RCH_ROW_STEPS - 1) t.tail_ok = false;
            }
            if (k > 0 && store_end > load_lo) t.overlay_ok = false;
            for (int i = 64 * k; i < 64 * k + 64; ++i) {
                const int end = (t.item[a][i] >> 8) * RCH_GP + 16 * (t.item[a][i] & 255) + 16;
                store_end = end > store_end ? end : store_end;
            }
        }
        // patch bytes: seven under every H value (LDS column 18 + a + ix - 3 + 3 .. + 6 = c + a .. c + a + 6), and the disc
        bool need[PS][PP] = {};
        for (int r = 0; r < PS; ++r)
            for (int c = 0; c < RCH_SIDE; ++c)
                if (H[r][c]) {
                    if (!it[r >> 1][(c + a) >> 2]) t.covered = false;
                    for (int k = 0; k < 7; ++k) need[r][c + a + k] = true;
                }
        for (int v = -15; v <= 15; ++v)
            for (int u = -umax[v < 0 ? -v : v]; u <= umax[v < 0 ? -v : v]; ++u) need[PR + v][PR + a + u] = true;
        n = 0;
        for (int r = 0; r < PS; ++r)
            for (int q = 0; q < 12; ++q)
                if (need[r][4 * q] || need[r][4 * q + 1] || need[r][4 * q + 2] || need[r][4 * q + 3]) {
                    if (n < 64 * RCH_STAGE_STEPS) t.dword[a][n] = (uint16_t)(r << 8 | q);
                    ++n;
                }
        for (int r = 0; r < PS; ++r)
            for (int c = 48; c < PP; ++c)
                if (need[r][c]) t.covered = false;  // past the twelve dwords the interior path stages
        t.n_dwords[a] = n;
        if (n > 64 * RCH_STAGE_STEPS || n == 0) t.fits = false;
        for (int i = n; i < 64 * RCH_STAGE_STEPS && n > 0; ++i) t.dword[a][i] = t.dword[a][n - 1];
    }
    return t;
}
constexpr Reach k_reach = reach_make();
static_assert(k_reach.fits, "reach: <= 192 row-pass items and <= 448 staged dwords per alignment, every pattern point within radius 18 x 18");
static_assert(k_reach.covered, "reach: every H value under the four dwords of a reachable sample lies inside a computed item, every needed byte inside the staged dwords");
static_assert(k_reach.overlay_ok, "reach: the plane bytes stored in steps 0 .. k lie below the first patch byte loaded in step k + 1");
static_assert(k_reach.tail_ok, "reach: the pair-row without an upper patch row belongs to the last step");

// Built by default: the trimmed ROW PASS.  The trimmed STAGING is built with -DDS_REACH_STAGING only: on the device it costs more than its two
// steps save (k_describe + 5 %: a lane's image address now waits for a table load, and the unpacking takes the vector instructions the steps
// gave back; DESIGN_LOG round 8).  -DDS_DENSE_PATCH: the dense staging and row pass of round 7 for every keypoint (A / B runs)
#if defined(DS_ROW_MAJOR_PLANE) || defined(DS_DENSE_PATCH)
#define DS_DENSE_ROWS
#undef DS_REACH_STAGING
#endif

// the per-lane tables.  Row pass: step k of lane l = item 64 k + l, packed as LDS byte offsets inside the slice: source (first of the three
// dwords of patch row 2 j) | destination << 16; a padding slot repeats the last item of its step (same loads, same store: harmless).
// Staging: step k of lane l = dword 64 k + l, packed as LDS byte offset of the dword inside the patch | patch row << 16
struct ReachRowTab {
    uint32_t e[4][64][4];
};
struct ReachStageTab {
    uint32_t e[4][64][8];
};
constexpr ReachRowTab reach_row_tab() {
    ReachRowTab t{};
    for (int a = 0; a < 4; ++a)
        for (int i = 0; i < 64 * RCH_ROW_STEPS; ++i) {
            const uint32_t j = k_reach.item[a][i] >> 8, g = k_reach.item[a][i] & 255;
            t.e[a][i & 63][i >> 6] = (RCH_P_OFF + 2 * j * PP + 4 * g) | (j * RCH_GP + 16 * g) << 16;
        }
    return t;
}
constexpr ReachStageTab reach_stage_tab() {
    ReachStageTab t{};
    for (int a = 0; a < 4; ++a)
        for (int i = 0; i < 64 * RCH_STAGE_STEPS; ++i) {
            const uint32_t r = k_reach.dword[a][i] >> 8, q = k_reach.dword[a][i] & 255;
            t.e[a][i & 63][i >> 6] = (r * PP + 4 * q) | r << 16;
        }
    return t;
}
#ifndef DS_DENSE_ROWS
__device__ __constant__ __attribute__((aligned(16))) const ReachRowTab k_reach_rows = reach_row_tab();
#endif
#ifdef DS_REACH_STAGING
__device__ __constant__ __attribute__((aligned(16))) const ReachStageTab k_reach_stage = reach_stage_tab();
#endif

#ifndef DS_DENSE_ROWS
static_assert(RCH_GP == GP && RCH_PAIR_ROWS == PAIR_ROWS && RCH_P_OFF == PLANE_BYTES - PS * PP, "reach tables: the slice layout of the kernel");
// the row pass over the items a BRIEF test can reach (alignment a, BRIEF centre = patch centre): per-item arithmetic as in blur_rows, the loads
// of step k + 1 before the store of step k; t = the lane's entry of k_reach_rows.  Plane entries outside the items keep stale bytes; nothing reads
// them (k_reach.covered)
__device__ __forceinline__ void blur_rows_reach(uint8_t *slice, const uint4 t) {
    const uint32_t ent[RCH_ROW_STEPS] = {t.x, t.y, t.z};
    const uint32_t *s0 = reinterpret_cast<const uint32_t *>(slice + (ent[0] & 0xffffu));
    uint32_t d[6] = {s0[0], s0[1], s0[2], s0[PP / 4], s0[PP / 4 + 1], s0[PP / 4 + 2]}, n[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < RCH_ROW_STEPS; ++k) {
        if (k + 1 < RCH_ROW_STEPS) {
            const uint32_t so = ent[k + 1] & 0xffffu;
            const uint32_t *s = reinterpret_cast<const uint32_t *>(slice + so);
            n[0] = s[0], n[1] = s[1], n[2] = s[2];
            // nothing past the slice is read: the last pair-row (last step only: k_reach.tail_ok) has no upper patch row; its u16 has weight 0
            if (k + 1 < RCH_ROW_STEPS - 1 || so < (uint32_t)(RCH_P_OFF + (PS - 1) * PP)) n[3] = s[PP / 4], n[4] = s[PP / 4 + 1], n[5] = s[PP / 4 + 2];
        }
        uint32_t e[4], o[4];
        row_taps4(d[0], d[1], d[2], e);
        row_taps4(d[3], d[4], d[5], o);
        uint4 w;
        w.x = e[0] | (o[0] << 16);
        w.y = e[1] | (o[1] << 16);
        w.z = e[2] | (o[2] << 16);
        w.w = e[3] | (o[3] << 16);
        *reinterpret_cast<uint4 *>(slice + (ent[k] >> 16)) = w;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = n[i];
    }
}
#endif

// host-only (no device, no context): the reach tables as the kernel holds them.  R: 37 x 37 bytes [iy + 18][ix + 18]; items[4][192]: pair-row << 8 |
// dword group in schedule order (step = index / 64, lane = index % 64), dwords[4][448]: patch row << 8 | dword of the row likewise, both padded
// with copies; counts[8]: items per alignment, staged dwords per alignment; layout[8]: row steps, staging steps, patch offset in the slice,
// patch pitch, bytes of a pair-row, slice bytes, 1 if the kernel trims the row pass, 1 if it trims the staging
extern "C" int afv_debug_describe_reach(uint8_t *R, uint16_t *items, uint16_t *dwords, int32_t *counts, int32_t *layout) {
    if (!R || !items || !dwords || !counts || !layout) return AFV_EINVAL;
    for (int y = 0; y < RCH_SIDE; ++y)
        for (int x = 0; x < RCH_SIDE; ++x) R[y * RCH_SIDE + x] = k_reach.R[y][x] ? 1 : 0;
    for (int a = 0; a < 4; ++a) {
        for (int i = 0; i < 64 * RCH_ROW_STEPS; ++i) items[a * 64 * RCH_ROW_STEPS + i] = k_reach.item[a][i];
        for (int i = 0; i < 64 * RCH_STAGE_STEPS; ++i) dwords[a * 64 * RCH_STAGE_STEPS + i] = k_reach.dword[a][i];
        counts[a] = k_reach.n_items[a];
        counts[4 + a] = k_reach.n_dwords[a];
    }
    layout[0] = RCH_ROW_STEPS, layout[1] = RCH_STAGE_STEPS, layout[2] = RCH_P_OFF, layout[3] = PP, layout[4] = RCH_GP;
    layout[5] = RCH_PAIR_ROWS * RCH_GP;
#ifdef DS_DENSE_ROWS
    layout[6] = 0;
#else
    layout[6] = 1;
#endif
#ifdef DS_REACH_STAGING
    layout[7] = 1;
#else
    layout[7] = 0;
#endif
    return AFV_OK;
}

// MODE 0: the extraction pipeline (keypoints of the quadtree survivors + their descriptors: detectAndCompute);
// MODE 1: keypoints only - position, IC angle, response (afv_orb_detect: detectKeypoints + filterKeypoints, Feature_orb32.cpp:26-40, :63-65);
// MODE 2: descriptors of CALLER-GIVEN keypoints at their own angle (afv_orb_compute: computeDescriptors = cv::ORB::compute, :42-53):
//         `given` holds total_blocks * KP_PER_BLOCK >= n keypoints of frame `frame_base`, `cap_per_frame` = n, descriptor i to desc[i]
template <int MODE>
__device__ __forceinline__ void describe_body(const Geo *__restrict__ geo_p, const FrameSrc src0, const uint8_t *__restrict__ pyr,
                                              const SelPoint *__restrict__ sel, const int *__restrict__ sel_count, afv_keypoint *__restrict__ kps,
                                              uint8_t *__restrict__ desc, int cap_per_frame, int *__restrict__ n_out, int *__restrict__ status,
                                              int frame_base, int per_frame, int total_blocks, const DescribeMirror mir,
                                              const afv_keypoint *__restrict__ given) {
    // One LDS slice per wavefront holds BOTH the staged patch (u8, rows PP = 52 bytes apart: 13 dwords, odd -> rows spread over all
    // LDS banks) and the row-filtered plane that is computed from it: the plane starts at byte 0, the patch ends where the slice ends
    // (byte P_OFF = SLICE - PS * PP on).  The row pass walks the plane upwards, ROW_LANES (pair-)rows per step, and within a step every
    // load precedes the store (DS operations of a wave execute in order; the loads of step k + 1 are even issued before the store of
    // step k), so all it takes is that the plane rows of steps 0 .. k end at or before the first patch row of step k + 1 begins:
    //   interleaved pairs: step k stores pair-rows < 6 (k + 1) = bytes < 960 (k + 1) and step k + 1 loads patch rows >= 12 (k + 1) = bytes
    //     >= 1284 + 624 (k + 1): 336 (k + 1) <= 1284 holds for k + 1 <= 3, the last step (the static_assert below checks every step);
    //   row-major u16: H row r ends before patch row r + 1 begins (80 r + 80 <= 1204 + 52 (r + 1) for r <= 42).
    // The plane fills the slice exactly, and nothing past the slice is read: the row pass skips the rows a step has past the patch (patch
    // row 43 would be the next wavefront's slice).  3520 (row-major: 3440) instead of 6028 bytes per keypoint: 14 080 bytes per workgroup,
    // 8 workgroups (all 32 wavefronts) per CU.  The patch is dead after the row pass: the IC moments are taken first, and the rare test of
    // a border keypoint that falls outside the level reads its (unblurred, reflected) pixel from the level image itself.
    constexpr int SLICE = PLANE_BYTES, P_OFF = SLICE - PS * PP;
    static_assert(P_OFF % 4 == 0 && P_OFF >= 0 && SLICE % 16 == 0, "slice layout");
#ifdef DS_ROW_MAJOR_PLANE
    static_assert(2 * HP * (PS - 1) + 2 * HP <= P_OFF + PP * PS, "H row r must end before patch row r + 1 begins");
#else
    constexpr bool overlap_ok = [] {
        for (int k = 0; k + 1 < ROW_STEPS; ++k)
            if (GP * ROW_LANES * (k + 1) > P_OFF + PP * 2 * ROW_LANES * (k + 1)) return false;
        return true;
    }();
    static_assert(overlap_ok, "the pair-rows of steps 0 .. k must end before the first patch row of step k + 1 begins");
    static_assert(PAIR_ROWS * GP == SLICE && 2 * PAIR_ROWS - 1 == PS, "pair-row 21 holds patch row 42 and a zero upper half");
    static_assert((PS - 1 - 6) / 2 + 3 < PAIR_ROWS, "a sample's four dwords (plane rows <= 36 + 6) lie inside the plane");
#endif
    static_assert(KP_PER_BLOCK * SLICE * 8 <= 160 * 1024, "8 workgroups per CU");
    __shared__ __attribute__((aligned(16))) uint8_t s_slice[KP_PER_BLOCK][SLICE];

    const Geo &geo = *geo_p;
    // the keypoint is a property of the wavefront: said so, its record, its patch origin and every per-keypoint scalar live on the scalar unit
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    int l = 0, f, out_idx, cx, cy;
    float given_angle = 0.f, resp = 0.f;
    if constexpr (MODE == 2) {
        // caller-given keypoints: wave i describes keypoint i.  BRIEF centre = cvRound(pt * (1 / scale)) in the keypoint's OWN octave
        // (orb.cpp computeOrbDescriptors; the host checked 0 <= octave < nlevels)
        f = frame_base;
        out_idx = (int)blockIdx.x * KP_PER_BLOCK + wv;
        if (out_idx >= cap_per_frame) return;  // wave-uniform
        const afv_keypoint g = given[out_idx];
        l = __builtin_amdgcn_readfirstlane(g.octave);
        const float inv = geo.lv[l].inv_scale;
        cx = __builtin_amdgcn_readfirstlane((int)rintf(g.x * inv));
        cy = __builtin_amdgcn_readfirstlane((int)rintf(g.y * inv));
        given_angle = g.angle;
    } else {
        // XCD-aware placement: all keypoints of a frame are described on one XCD (their patches share L2 lines)
        const int work = afv_xcd_remap(blockIdx.x, total_blocks);
        if (work >= total_blocks) return;
        // a frame's blocks: level after level, ceil(sel_cap / KP_PER_BLOCK) blocks each (per_frame in total)
        const int fl = (int)afv_udiv((uint32_t)work, geo.dv_desc_per_frame);
        const int blk = work - fl * per_frame;
#pragma unroll
        for (int i = 1; i < AFV_MAX_LEVELS; ++i)
            if (i < geo.nlevels && blk >= geo.lv[i].desc_blk_base) l = i;
        const int kblk = blk - geo.lv[l].desc_blk_base;
        f = frame_base + fl;
        const int idx = kblk * KP_PER_BLOCK + wv;

        // frame-level bookkeeping: counts of the eight levels (scalar loads), this level's first output slot, total
        const int4 *scp = reinterpret_cast<const int4 *>(sel_count + f * AFV_MAX_LEVELS);
        const int4 ca_ = scp[0], cb_ = scp[1];
        const int cnt[AFV_MAX_LEVELS] = {ca_.x, ca_.y, ca_.z, ca_.w, cb_.x, cb_.y, cb_.z, cb_.w};
        int level_base = 0, total = 0, mine = 0;
#pragma unroll
        for (int i = 0; i < AFV_MAX_LEVELS; ++i) {
            const int c = i < geo.nlevels ? cnt[i] : 0;
            level_base += i < l ? c : 0;
            mine = i == l ? c : mine;
            total += c;
        }
        if (blk == 0 && threadIdx.x == 0) {
            n_out[f] = min(total, cap_per_frame);
            if (mir.n) mir.n[f] = min(total, cap_per_frame);
            if (status && total > cap_per_frame) atomicMin(status, AFV_ECAPACITY);
        }
        if (idx >= mine) return;  // wave-uniform
        out_idx = level_base + idx;
        if (out_idx >= cap_per_frame) return;

        const SelPoint sp = sel[(size_t)f * geo.sel_per_frame + geo.lv[l].sel_base + idx];
        cx = sp.x;
        cy = sp.y;
        resp = sp.response;
    }
    const LevelGeo &L = geo.lv[l];
    const int lw = L.w, lh = L.h;
    const uint8_t *img;
    int pitch;
    if (l == 0) {
        img = src0.base + (size_t)f * src0.frame_stride;
        pitch = src0.stride;
    } else {
        img = pyr + L.pyr_off + (size_t)f * L.pyr_frame_stride;
        pitch = L.pitch;
    }
    uint8_t *P = s_slice[wv] + P_OFF;
    uint8_t *H = s_slice[wv];  // the row-filtered plane

    // ---- 1. stage the 43x43 unblurred patch; P[r][a + c] = level(cx-21+c, cy-21+r) with reflect-101 ----
    const int px0 = cx - PR, py0 = cy - PR;
    const bool interior = px0 >= 0 && py0 >= 0 && px0 + 48 <= lw && py0 + PS <= lh;  // wave-uniform
    const int a = interior ? px0 & 3 : 0;  // column offset of patch column 0 inside the LDS row: interior patches are staged as aligned dwords
#ifndef DS_DENSE_ROWS
    // the lane's three row-pass items, asked for before the patch: the load's latency passes behind the staging's
    uint4 row_items = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE != 1) row_items = *reinterpret_cast<const uint4 *>(k_reach_rows.e[a][lane]);
#endif
#ifndef DS_DENSE_PATCH
    // so are the lane's disc masks of the IC stage (the table loads of this kernel depend on the lane alone: each one issued where it is used
    // is a wait of a whole memory round trip per keypoint - round 8)
    uint4 mk = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE != 2) mk = *reinterpret_cast<const uint4 *>(k_ic_masks.m[lane]);
#endif
    // BRIEF centre = cvRound(pt * (1/scale)) with pt = level coordinate * scale (orb.cpp computeOrbDescriptors); a given keypoint's
    // centre IS that rounding already
    const float ptx = (float)cx * L.scale, pty = (float)cy * L.scale;
    const int bx = MODE == 2 ? cx : (int)rintf(ptx * L.inv_scale), by = MODE == 2 ? cy : (int)rintf(pty * L.inv_scale);
    const int ox = bx - cx, oy = by - cy;  // 0 in practice; kept literal
    // the reach tables hold for a BRIEF centre that is the patch centre; any other keypoint takes the dense staging and row pass (wave-uniform)
    const bool centred = (ox | oy) == 0;
#ifdef DS_REACH_STAGING
    // pitch >= PP: the table's LDS offset r * PP + 4 q becomes the image offset by adding r * (pitch - PP), one 24-bit multiply-add
    if (MODE != 1 && interior && centred && pitch >= PP) {
        // interior, staged for a descriptor: only the dwords the row pass and the IC disc read (k_reach), 64 per wave instruction
        const uint4 *tp = reinterpret_cast<const uint4 *>(k_reach_stage.e[a][lane]);
        const uint4 ta = tp[0], tb = tp[1];
        const uint32_t ent[RCH_STAGE_STEPS] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z};
        // 32-bit byte offsets from a scalar base, as below
        uint32_t o_patch = (uint32_t)py0 * (uint32_t)pitch + (uint32_t)(px0 - a), dp = (uint32_t)(pitch - PP);
        asm("" : "+s"(o_patch), "+s"(dp));
        const uint8_t *ip = img + o_patch;
        uint32_t v[RCH_STAGE_STEPS];  // loads first, then the LDS writes
#pragma unroll
        for (int k = 0; k < RCH_STAGE_STEPS; ++k) v[k] = *reinterpret_cast<const uint32_t *>(ip + mad_u24(ent[k] >> 16, dp, ent[k] & 0xffffu));
#pragma unroll
        for (int k = 0; k < RCH_STAGE_STEPS; ++k) *reinterpret_cast<uint32_t *>(P + (ent[k] & 0xffffu)) = v[k];
    } else
#endif
    if (interior) {
        // interior: 12 aligned dwords per row, 5 rows per wave instruction
        const int ax0 = px0 - a;
        const int rr = lane / 12, rq = lane - rr * 12;
        if (lane < 60) {
            // 32-bit byte offsets into the level image (a level is far below 4 GB; scalar base + vector offset is what the load takes):
            // the patch origin on the scalar unit, the lane's part by a 24-bit multiply, the row steps by scalar adds - no 64-bit
            // vector multiply-adds (quarter rate) in the address chain
            uint32_t o_patch = (uint32_t)py0 * (uint32_t)pitch + (uint32_t)ax0, o_step = 5u * (uint32_t)pitch;
            asm("" : "+s"(o_patch), "+s"(o_step));  // opaque scalars: the compiler would re-form (py0 + rr + 5 k) * pitch per row
            uint32_t o = o_patch + __umul24((uint32_t)rr, (uint32_t)pitch) + (uint32_t)(rq * 4);
            uint8_t *lp = &P[rr * PP + rq * 4];
            uint32_t v[9];  // rows rr, rr + 5, ..., rr + 40 (PS = 43: the last one exists for rr < 3): loads first, then the LDS writes
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (k < 8 || rr < PS - 40) v[k] = *reinterpret_cast<const uint32_t *>(img + o);
                o += o_step;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (k < 8 || rr < PS - 40) *reinterpret_cast<uint32_t *>(lp + k * 5 * PP) = v[k];
        }
    } else {
        // border: lane = patch column (reflected once), rows reflected per iteration (wave-uniform)
        if (lane < PS) {
            const int x = afv_reflect101(px0 + lane, lw);
            for (int r = 0; r < PS; ++r) {
                const int y = afv_reflect101(py0 + r, lh);  // wave-uniform
                P[r * PP + lane] = img[(uint32_t)y * (uint32_t)pitch + (uint32_t)x];
            }
        }
    }
    wave_sync();  // each wave owns its LDS slice: no workgroup barrier anywhere in this kernel

    // ---- 2. intensity centroid over the radius-15 disc: lane = (row, half) ----
    int m10 = 0, m01 = 0;
    if constexpr (MODE != 2) {
        const int v = (lane >> 1) - 15;  // -15..16
        if (v <= 15) {
            // half 0: u in [-d, -1] = bytes j = 16-d .. 15 of the 16 bytes starting at u = -16; half 1: u in [0, d] = bytes
            // j = 0 .. d of the 16 bytes starting at u = 0 (d = umax[|v|]).  Five aligned dwords, funnel-shifted to the start byte, bytes
            // outside the disc masked to zero (k_ic_masks), then sum(val) and sum(j * val) by v_dot4_u32_u8.
            const int half = lane & 1;
            const int A = (PR + v) * PP + PR + a + (half ? 0 : -16);
            const uint32_t *wp = reinterpret_cast<const uint32_t *>(P + (A & ~3));
            const int sh = (A & 3) * 8;
#ifdef DS_DENSE_PATCH
            const uint4 mk = *reinterpret_cast<const uint4 *>(k_ic_masks.m[lane]);
#endif
            const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4];
            const uint32_t b[4] = {__builtin_amdgcn_alignbit(w1, w0, sh) & mk.x, __builtin_amdgcn_alignbit(w2, w1, sh) & mk.y,
                                   __builtin_amdgcn_alignbit(w3, w2, sh) & mk.z, __builtin_amdgcn_alignbit(w4, w3, sh) & mk.w};
            uint32_t s1 = 0, sj = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s1 = __builtin_amdgcn_udot4(b[q], 0x01010101u, s1, false);
                sj = __builtin_amdgcn_udot4(b[q], 0x03020100u + 0x04040404u * (uint32_t)q, sj, false);
            }
            m10 = half ? (int)sj : (int)sj - 16 * (int)s1;
            m01 = v * (int)s1;
        }
    }
    // the row pass overwrites the patch (see the slice layout above): everything that reads P comes before these lines
#ifndef DS_DENSE_ROWS
    if constexpr (MODE != 1) {
        if (centred) blur_rows_reach(s_slice[wv], row_items);
        else blur_rows(P, H, lane);
    }
#else
    if constexpr (MODE != 1) blur_rows(P, H, lane);
#endif
    // the first group's test pairs, asked for before the angle is worked out; every later group's while the group before it is evaluated
    const float4 *pat = reinterpret_cast<const float4 *>(k_brief_pattern) + lane;
#ifndef DS_DENSE_PATCH
    float4 pt_next = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MODE != 1) pt_next = pat[0];
#endif
    float angle = given_angle;
    if constexpr (MODE != 2) {
        m10 = afv_wave_sum(m10);
        m01 = afv_wave_sum(m01);
        angle = fast_atan2_deg((float)m01, (float)m10);
    }
    if constexpr (MODE == 1) {  // keypoints only
        if (lane == 0) {
            afv_keypoint k;
            k.x = ptx;
            k.y = pty;
            k.size = 31 * L.scale;
            k.angle = angle;
            k.response = resp;
            k.octave = l;
            k.class_id = -1;
            kps[(size_t)f * cap_per_frame + out_idx] = k;
        }
        return;
    }

    // ---- 3+4. rotated BRIEF on the blurred patch: lane handles tests lane, lane+64, lane+128, lane+192; the blur is
    // evaluated only where a test samples it (512 of the 1369 patch positions) ----
    float ca, sb;
    sincos_deg(angle, ca, sb);
    wave_sync();  // row-filtered plane complete
    const int kox = ox - 0x4B400000, koy = oy - 0x4B400000;  // scalar: the mantissa offset of the rounding trick below and the (0) centre offset
    // a patch inside the level whose BRIEF centre is the patch centre (always, see above): LDS addresses straight from the float bits
    const bool direct = interior && centred;  // wave-uniform
    uint32_t k_addr = blur_addr_const((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)H, a);
    asm("" : "+s"(k_addr));  // one opaque scalar: the compiler would take it apart again and add its pieces per sample
    uint32_t words[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#ifdef DS_DENSE_PATCH
        const float4 pt = pat[g * 64];
#else
        const float4 pt = pt_next;
        if (g + 1 < 4) pt_next = pat[(g + 1) * 64];
#endif
        const float x0 = pt.x, y0 = pt.y, x1 = pt.z, y1 = pt.w;
        // (x ca - y sb, x sb + y ca) in PLAIN fp32, one rounding per operator (a - b = a + (-b), (-s) y = -(s y); -ffp-contract=off).
        // Round 5 held this as three packed instructions per point ((x, x) * (ca, sb) + (y, y) * (-sb, ca)); round 6 found that
        // v_pk_mul_f32 with a broadcast of its second operand's register (op_sel / op_sel_hi) returns the product of the OTHER register
        // in lanes 48..63 now and then while a wavefront of an MFMA kernel of another queue shares the SIMD (one wrong descriptor in a
        // few hundred frames beside k_match_topk_mfma; tools/probes/probe_pk_real.hip reproduces it in seconds, DESIGN_LOG round 6).
        // The whole library is built without packed fp32 instructions (build.py); this kernel does not ask for them either.
        const float rx0 = x0 * ca + y0 * -sb, ry0 = x0 * sb + y0 * ca, rx1 = x1 * ca + y1 * -sb, ry1 = x1 * sb + y1 * ca;
        // cvRound = round half to even: x + 1.5 * 2^23 leaves the rounded integer in the mantissa (|x| < 2^22; the addition rounds to
        // nearest even exactly where rintf does), one add per coordinate instead of v_rndne + v_cvt; the integer offset 0x4B400000
        // folds into the address constant (direct) or is taken off with the centre offset (border)
        const float rmag = 12582912.0f;
        const int fx0 = __float_as_int(rx0 + rmag), fy0 = __float_as_int(ry0 + rmag);
        const int fx1 = __float_as_int(rx1 + rmag), fy1 = __float_as_int(ry1 + rmag);
        // inside the ROI -> blurred, outside -> unblurred apron (a patch that lies inside the level has no outside samples)
        int t0, t1;
        if (direct) {
            t0 = blur_bits(fx0, fy0, k_addr);
            t1 = blur_bits(fx1, fy1, k_addr);
        } else {
            const int ix0 = fx0 + kox, iy0 = fy0 + koy, ix1 = fx1 + kox, iy1 = fy1 + koy;
            const int gx0 = cx + ix0, gy0 = cy + iy0, gx1 = cx + ix1, gy1 = cy + iy1;
            t0 = (gx0 >= 0 && gx0 < lw && gy0 >= 0 && gy0 < lh) ? blur_at(H, PR + a + ix0, PR + iy0)
                                                                 : (int)img[__umul24((uint32_t)afv_reflect101(gy0, lh), (uint32_t)pitch) + (uint32_t)afv_reflect101(gx0, lw)];
            t1 = (gx1 >= 0 && gx1 < lw && gy1 >= 0 && gy1 < lh) ? blur_at(H, PR + a + ix1, PR + iy1)
                                                                 : (int)img[__umul24((uint32_t)afv_reflect101(gy1, lh), (uint32_t)pitch) + (uint32_t)afv_reflect101(gx1, lw)];
        }
        const unsigned long long m = __ballot(t0 < t1);
        words[2 * g] = (uint32_t)m;
        words[2 * g + 1] = (uint32_t)(m >> 32);
    }
    // ---- 5. outputs (E11 merge: ascending level, list order inside a level) ----
    const size_t o = MODE == 2 ? (size_t)out_idx : (size_t)f * cap_per_frame + out_idx;
    if (lane < 8) {
        uint32_t w = words[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (lane == i) w = words[i];
        reinterpret_cast<uint32_t *>(desc + o * 32)[lane] = w;
        if (mir.desc) reinterpret_cast<uint32_t *>(mir.desc + o * 32)[lane] = w;  // afv_frame_extract: the frame's device copy
    }
    if (MODE == 0 && lane == 0) {
        afv_keypoint k;
        k.x = ptx;
        k.y = pty;
        k.size = 31 * L.scale;
        k.angle = angle;
        k.response = resp;
        k.octave = l;
        k.class_id = -1;
        kps[o] = k;
        if (mir.kps) mir.kps[o] = k;
    }
}

__global__ __launch_bounds__(64 * KP_PER_BLOCK) void k_describe(const Geo *__restrict__ geo_p, FrameSrc src0, const uint8_t *__restrict__ pyr,
                                                                const SelPoint *__restrict__ sel, const int *__restrict__ sel_count,
                                                                afv_keypoint *__restrict__ kps, uint8_t *__restrict__ desc, int cap_per_frame,
                                                                int *__restrict__ n_out, int *__restrict__ status, int frame_base, int per_frame,
                                                                int total_blocks, DescribeMirror mir) {
    describe_body<0>(geo_p, src0, pyr, sel, sel_count, kps, desc, cap_per_frame, n_out, status, frame_base, per_frame, total_blocks, mir, nullptr);
}
__global__ __launch_bounds__(64 * KP_PER_BLOCK) void k_describe_angles(const Geo *__restrict__ geo_p, FrameSrc src0, const uint8_t *__restrict__ pyr,
                                                                       const SelPoint *__restrict__ sel, const int *__restrict__ sel_count,
                                                                       afv_keypoint *__restrict__ kps, int cap_per_frame, int *__restrict__ n_out,
                                                                       int *__restrict__ status, int frame_base, int per_frame, int total_blocks) {
    describe_body<1>(geo_p, src0, pyr, sel, sel_count, kps, nullptr, cap_per_frame, n_out, status, frame_base, per_frame, total_blocks,
                     DescribeMirror{nullptr, nullptr, nullptr}, nullptr);
}
__global__ __launch_bounds__(64 * KP_PER_BLOCK) void k_describe_given(const Geo *__restrict__ geo_p, FrameSrc src0, const uint8_t *__restrict__ pyr,
                                                                      const afv_keypoint *__restrict__ given, int n, uint8_t *__restrict__ desc,
                                                                      int frame) {
    describe_body<2>(geo_p, src0, pyr, nullptr, nullptr, nullptr, desc, n, nullptr, nullptr, frame, 0, 0, DescribeMirror{nullptr, nullptr, nullptr}, given);
}

extern "C" int afv_describe_blocks_per_frame(const Geo *g) {
    int n = 0;
    for (int l = 0; l < g->nlevels; ++l) n += (g->lv[l].sel_cap + KP_PER_BLOCK - 1) / KP_PER_BLOCK;
    return n;
}

// `desc` == nullptr: keypoints only (afv_orb_detect)
extern "C" void afv_launch_describe(const Geo *geo_dev, int blocks_per_frame, const FrameSrc *src0, const uint8_t *pyr,
                                    const SelPoint *sel, const int *sel_count, afv_keypoint *kps, uint8_t *desc,
                                    int cap_per_frame, int *n_out, int *status, int frame_base, int nframes, const DescribeMirror *mirror,
                                    hipStream_t stream) {
    const int total = blocks_per_frame * nframes;
    dim3 grid((total + 7) / 8 * 8);
    if (!desc) {
        hipLaunchKernelGGL(k_describe_angles, grid, dim3(64 * KP_PER_BLOCK), 0, stream, geo_dev, *src0, pyr, sel, sel_count, kps, cap_per_frame, n_out,
                           status, frame_base, blocks_per_frame, total);
        return;
    }
    const DescribeMirror mir = mirror ? *mirror : DescribeMirror{nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_describe, grid, dim3(64 * KP_PER_BLOCK), 0, stream, geo_dev, *src0, pyr, sel, sel_count, kps, desc,
                       cap_per_frame, n_out, status, frame_base, blocks_per_frame, total, mir);
}

// descriptors of n caller-given keypoints (device array) on the pyramid of frame `frame`
extern "C" void afv_launch_describe_given(const Geo *geo_dev, const FrameSrc *src0, const uint8_t *pyr, const afv_keypoint *given, int n, uint8_t *desc,
                                          int frame, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_describe_given, dim3((n + KP_PER_BLOCK - 1) / KP_PER_BLOCK), dim3(64 * KP_PER_BLOCK), 0, stream, geo_dev, *src0, pyr, given, n, desc,
                       frame);
}

// ---------------- standalone E9: blur one level of one frame (debug / parity of the blur arithmetic) ----------------
__global__ __launch_bounds__(256) void k_blur_level(const uint8_t *__restrict__ img, int w, int h, int pitch,
                                                    uint8_t *__restrict__ out) {
    __shared__ uint8_t t[(16 + 6) * 72];
    __shared__ uint16_t hh[(16 + 6) * 64];
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 16;
    for (int i = threadIdx.x; i < 22 * 70; i += 256) {
        const int r = i / 70, c = i - r * 70;
        const int y = min(max(afv_reflect101(y0 + r - 3, h), 0), h - 1), x = min(max(afv_reflect101(x0 + c - 3, w), 0), w - 1);
        t[r * 72 + c] = img[(size_t)y * pitch + x];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 22 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        const uint8_t *p = &t[r * 72 + c];
        hh[r * 64 + c] = (uint16_t)(18 * (p[0] + p[6]) + 34 * (p[1] + p[5]) + 49 * (p[2] + p[4]) + 55 * p[3]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        const uint16_t *q = &hh[r * 64 + c];
        const int S = 18 * ((int)q[0] + q[6 * 64]) + 34 * ((int)q[64] + q[5 * 64]) + 49 * ((int)q[2 * 64] + q[4 * 64]) + 55 * (int)q[3 * 64];
        if (x0 + c < w && y0 + r < h) out[(size_t)(y0 + r) * w + x0 + c] = (uint8_t)blur_round((uint32_t)S);
    }
}

extern "C" void afv_launch_blur_level(const uint8_t *img, int w, int h, int pitch, uint8_t *out, hipStream_t stream) {
    dim3 grid((w + 63) / 64, (h + 15) / 16);
    hipLaunchKernelGGL(k_blur_level, grid, dim3(256), 0, stream, img, w, h, pitch, out);
}

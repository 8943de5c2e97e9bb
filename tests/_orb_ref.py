"""plain restatement of the numeric half of the ORB32 extractor (test infrastructure): umax, the intensity-centroid moments, cv::fastAtan2, the
cos / sin of rBRIEF, the 8U separable 7 x 7 Gaussian, rBRIEF itself and the Harris response - numpy and Python integers, written from the published
algorithms (OpenCV's orb.cpp / mathfuncs_core / the 8U separable filter) and the reference's FeatureExtractor.h:177-217, ORBextractor.cc:124-170 and
Feature_orb32.cpp.  Imports nothing from the library or the oracle; the only shared datum is the pattern table oracle/brief_pattern.inc, read as text.

Every rule a scene of tests/_desc_scenes.py targets is a field of `Rules` with deliberately WRONG alternatives next to the right value; the wrong ones exist
only so that tests/test_orb_ref_cpu.py can prove that the scene built for a rule changes when the rule does.

sincos = "double" needs mpmath (CPU tests only); everything else, `sincos_f64` (the scene generators' search helper) included, is numpy alone."""
import math
import os
import re
from collections import namedtuple

import numpy as np

f32 = np.float32
HALF_PATCH = 15

Rules = namedtuple("Rules", "blur_round compare disc sincos saturate atan_branch")
RIGHT = Rules(blur_round="half_even", compare="<", disc=0, sincos="double", saturate=True, atan_branch=">=")
ALTERNATIVES = {"blur_round": ("half_up", "truncate"), "compare": ("<=",), "disc": (1, -1), "sincos": ("float32",), "saturate": (False,),
                "atan_branch": (">",)}


def reflect101(p, n):
    """BORDER_REFLECT_101 index (arrays welcome): ... 2 1 | 0 1 2 ... n-2 n-1 | n-2 n-3 ..."""
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    m = 2 * n - 2
    p = np.mod(p, m)
    return np.where(p >= n, m - p, p)


def umax():
    """last column of row v = 0..15 of the radius-15 disc: round(sqrt(15^2 - v^2)) up to the 45 degree row, the rest mirrored so that the disc is
    symmetric under a swap of u and v (ORBextractor.cc:124-139).  sqrt of a non-square is never n + 0.5: floor(sqrt(n) + 0.5) = (isqrt(4 n) + 1) // 2."""
    hp = HALF_PATCH
    vmax = math.floor(hp * math.sqrt(2.0) / 2 + 1)
    vmin = math.ceil(hp * math.sqrt(2.0) / 2)
    u = [0] * (hp + 1)
    for v in range(vmax + 1):
        u[v] = (math.isqrt(4 * (hp * hp - v * v)) + 1) // 2
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u


UMAX = umax()


def moments(level, x, y, rules=RIGHT):
    """(m10, m01) of the disc centred on (x, y), exact integers; pixels outside the level are the reflected ones"""
    h, w = level.shape
    m10 = m01 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = UMAX[abs(v)] + rules.disc
        us = np.arange(-d, d + 1)
        row = level[int(reflect101(y + v, h)), reflect101(x + us, w)].astype(np.int64)
        m10 += int((us * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


_RAD2DEG = f32(180.0 / 3.1415926535897932384626433832795)
_P1, _P3, _P5, _P7 = (f32(c) * _RAD2DEG for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))
_EPS = f32(2.220446049250313e-16)  # (float)DBL_EPSILON


def fast_atan2(y, x, rules=RIGHT):
    """cv::fastAtan2 in degrees, every operation rounded to float32 once"""
    y, x = f32(y), f32(x)
    ax, ay = abs(x), abs(y)
    first = ax >= ay if rules.atan_branch == ">=" else ax > ay
    if first:
        c = ay / (ax + _EPS)
        c2 = c * c
        a = (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    else:
        c = ax / (ay + _EPS)
        c2 = c * c
        a = f32(90.0) - (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    if x < 0:
        a = f32(180.0) - a
    if y < 0:
        a = f32(360.0) - a
    return f32(a)


def ic_angle(level, x, y, rules=RIGHT):
    m10, m01 = moments(level, x, y, rules)
    return fast_atan2(f32(m01), f32(m10), rules)


FACTOR_PI = f32(3.1415926535897932384626433832795 / 180.0)  # (float)(CV_PI / 180.f), FeatureExtractor.h:177


def _sincos_f32(t):
    """the WRONG alternative: cos / sin evaluated in float32 throughout (reduction by a float32 pi / 2, Taylor sums in float32); arrays welcome"""
    t = np.asarray(t, f32)
    k = np.rint(t * f32(2.0 / math.pi))
    r = (t - k * f32(math.pi / 2)).astype(f32)
    z = r * r
    c, s = np.zeros_like(r), np.zeros_like(r)
    for n in range(14, -1, -2):  # Horner: cos = sum (-1)^(n/2) r^n / n!, sin = r * sum (-1)^(n/2) r^n / (n + 1)!
        sign = 1.0 if n % 4 == 0 else -1.0
        c = c * z + f32(sign / math.factorial(n))
        s = s * z + f32(sign / math.factorial(n + 1))
    s = s * r
    q = k.astype(np.int64) & 3
    return np.choose(q, [c, -s, -c, s]).astype(f32), np.choose(q, [s, c, -s, -c]).astype(f32)


def sincos_f64(angle_deg):
    """numpy only: cos / sin in float64 by the platform's libm, cast to float32 (arrays welcome).  The scene generators SEARCH with it; what the
    scenes are checked against is sincos() below."""
    t = (np.asarray(angle_deg, f32) * FACTOR_PI).astype(np.float64)
    return np.cos(t).astype(f32), np.sin(t).astype(f32)


_sincos_memo = {}


def sincos(angle_deg, rules=RIGHT):
    """memo of _sincos on the angle's BITS (-0 and +0 are different inputs)"""
    key = (int(f32(angle_deg).view(np.uint32)), rules.sincos)
    if key not in _sincos_memo:
        _sincos_memo[key] = _sincos(angle_deg, rules)
    return _sincos_memo[key]


def _sincos(angle_deg, rules):
    """(cos, sin) as FeatureExtractor.h:182-183 evaluates them: angle * factorPI is a float product, cos and sin of it are taken in double and cast to
    float - i.e. the exact value (120 bits here) rounded to double, then to float"""
    t = f32(f32(angle_deg) * FACTOR_PI)
    if rules.sincos == "float32":
        c, s = _sincos_f32(t)
        return f32(c), f32(s)  # 0-d arrays -> scalars
    import mpmath
    out = []
    with mpmath.workprec(120):
        exact = (mpmath.cos(mpmath.mpf(float(t))), mpmath.sin(mpmath.mpf(float(t))))
        for v in exact:
            with mpmath.workprec(53):
                d = +v  # round to nearest, ties to even, 53 bits (no double of this size is subnormal)
            out.append(f32(np.float64(float(d))))
    if out[1] == 0:
        out[1] = f32(np.copysign(0.0, t))  # sin(-0) is -0 in IEEE arithmetic; mpmath has no signed zero
    return out[0], out[1]


def gauss_taps():
    """7 taps of sigma 2 as the 8U separable filter uses them: float kernel * 256, rounded"""
    g = [math.exp(-(i - 3) ** 2 / (2.0 * 2.0 * 2.0)) for i in range(7)]
    s = sum(g)
    return [int(np.rint(np.float64(f32(v / s)) * 256.0)) for v in g]


TAPS = gauss_taps()


def blur_sums(level):
    """S of every pixel: exact integer row and column passes over a reflect-101 border"""
    h, w = level.shape
    p = level.astype(np.int64)[reflect101(np.arange(-3, h + 3), h)][:, reflect101(np.arange(-3, w + 3), w)]
    rows = sum(TAPS[k] * p[:, k:k + w] for k in range(7))
    return sum(TAPS[k] * rows[k:k + h] for k in range(7))


def blur_round(S, rules=RIGHT):
    S = np.asarray(S, np.int64)
    q, r = S >> 16, S & 0xFFFF
    if rules.blur_round == "half_even":
        q = q + ((r > 32768) | ((r == 32768) & (q & 1 == 1)))
    elif rules.blur_round == "half_up":
        q = q + (r >= 32768)
    else:
        assert rules.blur_round == "truncate"
    return (np.minimum(q, 255) if rules.saturate else q & 255).astype(np.uint8)


def blur(level, rules=RIGHT):
    return blur_round(blur_sums(level), rules)


def brief_pattern():
    """256 x (x0, y0, x1, y1) from the committed table"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "brief_pattern.inc")
    with open(path) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    v = np.array([int(t) for t in re.findall(r"-?\d+", text)], np.int32)
    assert v.size == 1024
    return v.reshape(256, 2, 2)


PATTERN = brief_pattern()


def rotate_pattern(a, b):
    """float32 (x a - y b, x b + y a) of all 512 points, one rounding per operator -> [256, 2, 2] float32 (x', y')"""
    a, b = f32(a), f32(b)
    x, y = PATTERN[..., 0].astype(f32), PATTERN[..., 1].astype(f32)
    return np.stack([x * a - y * b, x * b + y * a], -1)


def sample_positions(angle_deg, rules=RIGHT):
    """cvRound (round half to even) of the rotated pattern -> [256, 2, 2] int (dx, dy)"""
    a, b = sincos(angle_deg, rules)
    return np.rint(rotate_pattern(a, b)).astype(np.int64)


def descriptor(level, blurred, cx, cy, angle_deg, rules=RIGHT):
    """rBRIEF at (cx, cy): a sample inside the level reads the blurred plane, one outside reads the UNBLURRED reflected apron"""
    h, w = level.shape
    pos = sample_positions(angle_deg, rules)
    gx, gy = cx + pos[..., 0], cy + pos[..., 1]
    inside = (gx >= 0) & (gx < w) & (gy >= 0) & (gy < h)
    val = np.where(inside, blurred[np.clip(gy, 0, h - 1), np.clip(gx, 0, w - 1)], level[reflect101(gy, h), reflect101(gx, w)]).astype(np.int64)
    bits = val[:, 0] < val[:, 1] if rules.compare == "<" else val[:, 0] <= val[:, 1]
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def harris_sums(level, x, y):
    """Sobel sums a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 block centred on (x, y): exact integers"""
    h, w = level.shape
    p = level.astype(np.int64)[reflect101(np.arange(y - 4, y + 5), h)][:, reflect101(np.arange(x - 4, x + 5), w)]
    ix = 2 * (p[1:8, 2:9] - p[1:8, 0:7]) + (p[0:7, 2:9] - p[0:7, 0:7]) + (p[2:9, 2:9] - p[2:9, 0:7])
    iy = 2 * (p[2:9, 1:8] - p[0:7, 1:8]) + (p[2:9, 0:7] - p[0:7, 0:7]) + (p[2:9, 2:9] - p[0:7, 2:9])
    return int((ix * ix).sum()), int((iy * iy).sum()), int((ix * iy).sum())


def harris_response(a, b, c):
    """((float)a * b - (float)c * c - k * ((float)a + b) * ((float)a + b)) * scale^4 in float32, left to right"""
    fa, fb, fc = f32(a), f32(b), f32(c)
    scale = f32(1.0) / (f32(4 * 7) * f32(255.0))
    s4 = scale * scale * scale * scale
    return f32((fa * fb - fc * fc - f32(0.04) * (fa + fb) * (fa + fb)) * s4)

"""a float64 restatement of the AKAZE61 scale space (test data, numpy only), written from the algorithm (Alcantarilla et al., "Fast
Explicit Diffusion for Accelerated Features in Nonlinear Scale Spaces", BMVC 2013), vectorised, not transcribed from oracle/akaze.c:

  * FED step sizes in closed form, tau_k = (s tau_max / 2) / cos^2(pi (2k + 1) / (4n + 2)), reordered by the kappa-cycle of the
    next prime >= n + 1 (kappa = n / 2);
  * Gaussian with replicated borders, Scharr [3 10 3] x [-1 0 1] with reflect-101 borders, the pm_g2 conductivity
    1 / (1 + |grad|^2 / k^2) and the explicit diffusion step L + tau/2 div(c grad L) with zero flux across the border;
  * 2x INTER_AREA (the mean of each 2 x 2 block);
  * the contrast factor: 70th percentile of the gradient magnitude histogram (300 bins over [0, hmax]);
  * the Hessian from sparse-tap Scharr derivatives at distance sigma_size, first derivatives scaled by sigma_size, second by sigma_size^2.
check_against_f64 holds a float32 computation (the oracle's or the kernels') to the bounds measured in tests/test_oracle_akaze_f64.py."""
import math

import numpy as np

TAU_MAX = 0.25

# Bounds: the oracle (float32, one rounding per operator) against this float64 restatement, measured on the scenes of
# tests/_akaze_scenes.py and seeded synth frames (tests/test_oracle_akaze_f64.py), then about doubled.  Errors are max |f32 - f64| over a
# level, relative to max |f64| of that level's plane.
BOUND_TAU = 4e-6         # relative error of a FED step; measured 1.6e-6
BOUND_PLANE = {          # measured (largest over levels and frames):
    "Lt": 1.2e-6,        # 5.5e-7
    "Lsmooth": 7e-7,     # 3.1e-7
    "Lx": 2.5e-6,        # 1.2e-6
    "Ly": 3.2e-6,        # 1.6e-6
    "Ldet": 5e-6,        # 2.3e-6
}
BOUND_KCONTRAST = 7e-7   # |k32 - k64| / hmax; measured 3.4e-7


def fed_tau(T, tau_max=TAU_MAX):
    """FED cycle that covers evolution time T: n = ceil(sqrt(3T / tau_max + 1/4) - 1/2) steps, closed form, kappa-cycle order"""
    n = int(math.ceil(math.sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1e-8))
    if n <= 0:
        return np.zeros(0)
    s = 3.0 * T / (tau_max * n * (n + 1))
    k = np.arange(n)
    tau = (s * tau_max / 2.0) / np.cos(np.pi * (2 * k + 1) / (4 * n + 2)) ** 2
    kappa, prime = n // 2, n + 1
    while any(prime % d == 0 for d in range(2, int(math.isqrt(prime)) + 1)):
        prime += 1
    order = [j - 1 for j in ((np.arange(1, prime) * kappa) % prime) if j - 1 < n and j >= 1][:n]
    return tau[order]


def gauss_taps(sigma):
    ks = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)))
    ks += 1 - ks % 2
    x = np.arange(ks) - (ks - 1) / 2.0
    t = np.exp(-x * x / (2.0 * sigma * sigma))
    return t / t.sum()


def _sep(img, kx, ky, mode):
    """separable correlation, rows then columns, border padding `mode` (numpy: 'edge' = replicate, 'reflect' = reflect-101)"""
    rx, ry = len(kx) // 2, len(ky) // 2
    p = np.pad(img, ((0, 0), (rx, rx)), mode=mode)
    t = sum(kx[j] * p[:, j:j + img.shape[1]] for j in range(len(kx)))
    p = np.pad(t, ((ry, ry), (0, 0)), mode=mode)
    return sum(ky[j] * p[j:j + img.shape[0], :] for j in range(len(ky)))


def gauss(img, sigma):
    k = gauss_taps(sigma)
    return _sep(img, k, k, "edge")


def scharr(img):
    d, s = np.array([-1.0, 0.0, 1.0]), np.array([3.0, 10.0, 3.0])
    return _sep(img, d, s, "reflect"), _sep(img, s, d, "reflect")


def halfsample(img):
    h, w = img.shape[0] // 2 * 2, img.shape[1] // 2 * 2
    a = img[:h, :w]
    return 0.25 * (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2])


def conductivity(lsmooth, k):
    lx, ly = scharr(lsmooth)
    return 1.0 / (1.0 + (lx * lx + ly * ly) / (k * k))


def nld_step(L, c, tau):
    """L + tau/2 * div(c grad L) with the face conductivities c_i + c_j and zero flux across the border"""
    fx = (c[:, 1:] + c[:, :-1]) * (L[:, 1:] - L[:, :-1])
    fy = (c[1:, :] + c[:-1, :]) * (L[1:, :] - L[:-1, :])
    div = np.zeros_like(L)
    div[:, :-1] += fx; div[:, 1:] -= fx
    div[:-1, :] += fy; div[1:, :] -= fy
    return L + 0.5 * tau * div


def grad_magnitude(img):
    g = gauss(img, 1.0)
    lx, ly = scharr(g)
    return np.sqrt(lx * lx + ly * ly)[1:-1, 1:-1]


def kcontrast(img, perc=0.7, nbins=300):
    """(contrast factor, magnitudes of the interior, hmax); hmax == 0 or too few points -> 0.03"""
    m = grad_magnitude(img)
    hmax = float(m.max()) if m.size else 0.0
    if hmax == 0.0:
        return 0.03, m, hmax
    nz = m[m != 0]
    b = np.minimum(np.floor(nbins * nz / hmax).astype(np.int64), nbins - 1)
    hist = np.bincount(b, minlength=nbins)
    nth = int(len(nz) * perc)
    cum = np.cumsum(hist)
    k = int(np.searchsorted(cum, nth)) + 1 if nth > 0 else 0
    if nth > 0 and cum[-1] < nth:
        return 0.03, m, hmax
    return hmax * k / nbins, m, hmax


def sparse_scharr(img, s, xorder):
    """d/dx (xorder) or d/dy of the Scharr kernel with taps at distance s, normalised by 1 / (2 s (10/3 + 2))"""
    w = 10.0 / 3.0
    norm = 1.0 / (2.0 * s * (w + 2.0))
    d = np.zeros(2 * s + 1); d[0], d[-1] = -1.0, 1.0
    sm = np.zeros(2 * s + 1); sm[0] = sm[-1] = norm; sm[s] = w * norm
    return _sep(img, d, sm, "reflect") if xorder else _sep(img, sm, d, "reflect")


def hessian(lsmooth, s):
    lx, ly = sparse_scharr(lsmooth, s, 1), sparse_scharr(lsmooth, s, 0)
    lxx, lyy, lxy = sparse_scharr(lx, s, 1), sparse_scharr(ly, s, 0), sparse_scharr(lx, s, 0)
    s2 = float(s * s)
    return lx * s, ly * s, (lxx * s2) * (lyy * s2) - (lxy * s2) ** 2


def scale_space(gray, plan, k0=None, soffset=1.6):
    """float64 planes of every level; k0: the contrast factor to diffuse with (default: the float64 one)"""
    img = np.asarray(gray, np.float64) / 255.0
    kc = kcontrast(img)[0] if k0 is None else float(k0)
    out = []
    lt = gauss(img, soffset)
    for i in range(plan.nlevels):
        L = plan.lv[i]
        if i == 0:
            ls = lt
        else:
            if L.octave > plan.lv[i - 1].octave:
                lt = halfsample(lt)
                kc = kc * 0.75
            ls = gauss(lt, 1.0)
            c = conductivity(ls, kc)
            for tau in fed_tau(L.etime - plan.lv[i - 1].etime):
                lt = nld_step(lt, c, tau)
        lx, ly, ldet = hessian(ls, L.sigma_size)
        out.append(dict(Lt=lt, Lsmooth=ls, Lx=lx, Ly=ly, Ldet=ldet))
    return out


def plane_errors(got, ref):
    """{plane: [relative max error per level]}"""
    return {n: [float(np.max(np.abs(g[n].astype(np.float64) - r[n])) / max(float(np.max(np.abs(r[n]))), 1e-30)) for g, r in zip(got, ref)]
            for n in BOUND_PLANE}


def kcontrast_bin_ok(gray, k32, perc=0.7, nbins=300):
    """k32 (float32 contrast factor) is hmax * k / nbins with the float64 k, or with k +- 1 only when the magnitudes that lie within
    BOUND_KCONTRAST of the boundary between the two bins are enough to move the cumulative count across the percentile threshold.
    Returns (ok, float64 value, was the neighbouring bin needed)"""
    img = np.asarray(gray, np.float64) / 255.0
    k64, m, hmax = kcontrast(img, perc, nbins)
    if hmax == 0.0 or k64 == 0.03:
        return np.float32(k32) == np.float32(0.03), k64, False
    if abs(float(k32) - k64) <= BOUND_KCONTRAST * hmax:
        return True, k64, False
    kb, kb32 = int(round(k64 * nbins / hmax)), int(round(float(k32) * nbins / hmax))
    if abs(kb32 - kb) != 1:
        return False, k64, False
    x = nbins * m[m != 0] / hmax
    edge = max(kb, kb32) - 1                        # the boundary between the two candidate bins, on the x = nbins * m / hmax scale
    below = int(np.count_nonzero(x < edge))           # magnitudes in the bins below the boundary
    near = int(np.count_nonzero(np.abs(x - edge) <= BOUND_KCONTRAST * nbins * 2))
    nth = int(len(x) * perc)
    # k = first bin whose cumulative count reaches nth, + 1: the count below the boundary decides between the two bins
    return abs(below - nth) <= near + 1, k64, True


def check_against_f64(gray, plan, got, k32):
    """assert that float32 planes `got` (list of dicts per level) and contrast factor k32 lie within the float64 bounds"""
    ok, k64, _ = kcontrast_bin_ok(gray, k32)
    assert ok, ("kcontrast", k32, k64)
    ref = scale_space(gray, plan, k0=np.float32(k32))
    err = plane_errors(got, ref)
    for n, bound in BOUND_PLANE.items():
        assert max(err[n]) <= bound, (n, err[n], bound)
    return err


# ---- Feature_Detection and Compute_Descriptors on the float64 planes ----
DTHRESHOLD = 0.0005
ORI_EDGE = 1e-5          # radians: a sample angle this close to a window edge is a decision of the float32 rounding
ORI_TIE = 1e-4           # two windows with different samples this close in |sum|^2 (relative) tie within the rounding (the SURF weight table
                         # of the oracle holds 8 decimals: up to 1.2e-4 relative on its smallest weights)
BOUND_ANGLE = 1e-6       # radians: the float32 angle against the float64 one where the window choice is clear; measured 4.6e-7
ROUND_EDGE = 1e-4        # pixels: a sample position this close to a rounding boundary may read the neighbouring pixel
BOUND_MLDB_SUM = 1e-5    # relative to the plane's largest value: float32 sums of up to 100 samples, n u = 6e-6


def candidates(ldet, sigma_size, eps):
    """strict 3 x 3 maxima above the threshold inside the descriptor border (raster order, as y * w + x); and the positions whose
    decision lies within eps of a comparison (excluded from the comparison)"""
    h, w = ldet.shape
    c = ldet[1:-1, 1:-1]
    nb = [ldet[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    is_max = c > DTHRESHOLD
    near = np.abs(c - DTHRESHOLD) <= eps
    for n in nb:
        is_max &= c > n
        near |= np.abs(c - n) <= eps
    ys, xs = np.mgrid[1:h - 1, 1:w - 1]
    reach = 10.0 * math.sqrt(2.0) * sigma_size
    inside = (np.floor(xs - reach + 0.5) - 1 >= 0) & (np.floor(xs + reach + 0.5) + 1 < w) & \
             (np.floor(ys - reach + 0.5) - 1 >= 0) & (np.floor(ys + reach + 0.5) + 1 < h)
    idx = ys * w + xs
    return idx[is_max & inside], idx[near & inside]


def subpixel(ldet, x, y, octave, eps):
    """the 2 x 2 solve of the quadratic fit around integer maxima (x, y arrays of the level): -> (keep, x0, y0 in level-0 pixels,
    position error bound in level-0 pixels, keep-decision is within the error)"""
    D = lambda dy, dx: ldet[y + dy, x + dx]
    g = np.stack([0.5 * (D(0, 1) - D(0, -1)), 0.5 * (D(1, 0) - D(-1, 0))], -1)
    dxx = D(0, 1) + D(0, -1) - 2.0 * D(0, 0)
    dyy = D(1, 0) + D(-1, 0) - 2.0 * D(0, 0)
    dxy = 0.25 * (D(1, 1) + D(-1, -1) - D(-1, 1) - D(1, -1))
    H = np.stack([np.stack([dxx, dxy], -1), np.stack([dxy, dyy], -1)], -2)
    det = dxx * dyy - dxy * dxy
    ok = det != 0
    Hs = np.where(ok[:, None, None], H, np.eye(2))
    d = -np.linalg.solve(Hs, g[..., None])[..., 0]
    inv = np.abs(np.linalg.inv(Hs)).sum(-1).max(-1)             # |H^-1| (max row sum)
    err = 2.0 * inv * 4.0 * eps * (1.0 + np.abs(d).sum(-1))       # first-order error of d for entries known to +-4 eps
    keep = ok & (np.abs(d) <= 1.0).all(-1)
    amb = ~ok | (np.abs(np.abs(d).max(-1) - 1.0) <= err)
    p = float(2 ** octave)
    return keep, (x + d[:, 0]) * p, (y + d[:, 1]) * p, err * p, amb


def _gauss25(i, j):
    return np.exp(-(i * i + j * j) / (2 * 2.5 * 2.5)) / (2 * np.pi * 2.5 * 2.5)


def orientation(lx, ly, xf, yf, s):
    """dominant orientation: Gaussian-weighted gradients of the 109 samples within radius 6 s, the 60-degree window swept in 0.15 rad
    steps, the angle of the largest summed vector.  -> (angle, ambiguous)"""
    h, w = lx.shape
    ij = np.array([(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j < 36])
    fx, fy = xf + ij[:, 0] * s + 0.5, yf + ij[:, 1] * s + 0.5
    px = np.clip(np.floor(fx).astype(int), 0, w - 1)
    py = np.clip(np.floor(fy).astype(int), 0, h - 1)
    on_edge = bool(np.any(np.abs(fx - np.rint(fx)) <= ROUND_EDGE) or np.any(np.abs(fy - np.rint(fy)) <= ROUND_EDGE))
    g = _gauss25(ij[:, 0], ij[:, 1])
    rx, ry = g * lx[py, px], g * ly[py, px]
    ang = np.mod(np.arctan2(ry, rx), 2 * np.pi)
    a1 = 0.15 * np.arange(int(np.ceil(2 * np.pi / 0.15)))
    a2 = np.mod(a1 + np.pi / 3, 2 * np.pi)
    wrap = a2 < a1
    A = ang[None, :]
    inside = np.where(wrap[:, None], (A > 0) & (A < a2[:, None]) | (A > a1[:, None]), (A > a1[:, None]) & (A < a2[:, None]))
    sx, sy = inside @ rx, inside @ ry
    val = sx * sx + sy * sy
    best = int(np.argmax(val))
    amb, tie = on_edge, False
    if val[best] > 0:
        others = [k for k in range(len(val)) if k != best and not np.array_equal(inside[k], inside[best])]
        tie = any(val[k] >= val[best] * (1 - ORI_TIE) for k in others)
        amb |= tie
        edges = np.concatenate([[a1[best], a2[best]]])
        amb |= bool(np.any(np.abs(ang[:, None] - edges[None, :]) <= ORI_EDGE))
    return (float(np.mod(np.arctan2(sy[best], sx[best]), 2 * np.pi)) if val[best] > 0 else 0.0), amb, tie


def mldb_values(lt, lx, ly, xf, yf, scale, angle):
    """the three MLDB grids (2 x 2, 3 x 3, 4 x 4 cells over a 20 x 20 pattern scaled by `scale`, rotated by `angle`): per grid an array
    (cells, 3) of the cell means of intensity and of the two rotated derivatives, and per grid the cells with a sample position within
    ROUND_EDGE of a rounding boundary"""
    h, w = lt.shape
    co, si = math.cos(angle), math.sin(angle)
    out = []
    for step in (10, 7, 5):
        vals, amb = [], []
        for i in range(-10, 10, step):
            for j in range(-10, 10, step):
                k, l = np.meshgrid(np.arange(i, i + step), np.arange(j, j + step), indexing="ij")
                sy = yf + (l * co + k * si) * scale
                sx = xf + (-l * si + k * co) * scale
                fy, fx = sy + 0.5, sx + 0.5
                amb.append(bool(np.any(np.abs(fy - np.rint(fy)) <= ROUND_EDGE) or np.any(np.abs(fx - np.rint(fx)) <= ROUND_EDGE)))
                qy = np.clip(np.floor(fy).astype(int), 0, h - 1)
                qx = np.clip(np.floor(fx).astype(int), 0, w - 1)
                rx, ry = lx[qy, qx], ly[qy, qx]
                vals.append([lt[qy, qx].mean(), (-rx * si + ry * co).mean(), (rx * co + ry * si).mean()])
        out.append((np.array(vals), np.array(amb)))
    return out


def mldb_bits(grids, eps3):
    """486 bits in the descriptor's order (per grid, per channel, all pairs i < j: value_i > value_j) and a mask of the bits that are
    decided by more than eps3[channel] and read no ambiguous cell"""
    bits, sure = [], []
    for vals, amb in grids:
        n = len(vals)
        for c in range(3):
            v = vals[:, c]
            for i in range(n):
                for j in range(i + 1, n):
                    bits.append(v[i] > v[j])
                    sure.append(abs(v[i] - v[j]) > eps3[c] and not amb[i] and not amb[j])
    return np.array(bits), np.array(sure)


def check_detection_f64(gray, plan, ref, cands32, unrefined32, refined32):
    """float32 candidates per level, the keypoints before and after the subpixel step, against the float64 detection on the float64
    planes `ref`.  Returns (items compared, items excluded because the float64 margin is within the bound)"""
    n_cmp = n_exc = 0
    for i in range(plan.nlevels):
        L = plan.lv[i]
        ldet = ref[i]["Ldet"]
        eps = 2.0 * BOUND_PLANE["Ldet"] * max(float(np.max(np.abs(ldet))), 1e-30)
        want, near = candidates(ldet, L.sigma_size, eps)
        got = np.asarray(cands32[i])
        sure = lambda a: a[~np.isin(a, near)]
        assert np.array_equal(np.sort(sure(got)), np.sort(sure(want))), ("candidates", i)
        n_cmp += len(np.union1d(got, want)); n_exc += len(np.intersect1d(np.union1d(got, want), near))
    for i in range(plan.nlevels):
        L = plan.lv[i]
        sel = unrefined32["class_id"] == i
        if not sel.any():
            continue
        ldet = ref[i]["Ldet"]
        eps = 2.0 * BOUND_PLANE["Ldet"] * max(float(np.max(np.abs(ldet))), 1e-30)
        r = float(2 ** L.octave)
        x = np.floor(unrefined32["x"][sel] / r + 0.5).astype(int)
        y = np.floor(unrefined32["y"][sel] / r + 0.5).astype(int)
        keep, x0, y0, err, amb = subpixel(ldet, x, y, L.octave, eps)
        got = refined32[refined32["class_id"] == i]
        # refined keypoints keep the order of the unrefined ones: walk both lists
        resp = unrefined32["response"][sel]
        k = 0
        for t in range(len(x)):
            # the refined list is the unrefined one with points dropped, in the same order; the response is carried over unchanged
            kept32 = k < len(got) and got["response"][k] == resp[t] and abs(got["x"][k] / r - x[t]) <= 1 and abs(got["y"][k] / r - y[t]) <= 1
            if amb[t]:
                n_exc += 1
            else:
                assert bool(keep[t]) == bool(kept32), ("subpixel keep", i, t, bool(keep[t]), x0[t], y0[t])
                if kept32:
                    assert abs(got["x"][k] - x0[t]) <= err[t] + 1e-4 and abs(got["y"][k] - y0[t]) <= err[t] + 1e-4, \
                        ("subpixel position", i, t, got[k], x0[t], y0[t], err[t])
                n_cmp += 1
            k += int(kept32)
        assert k == len(got), ("subpixel: float32 keeps points the float64 step drops", i, k, len(got))
    return n_cmp, n_exc


def check_descriptors_f64(plan, ref, kps32, desc32):
    """angles and MLDB bits of float32 features against the float64 orientation and MLDB on the float64 planes.  The MLDB bits are
    computed with the float32 angle (so that a near-tie of the orientation does not hide the MLDB).  Returns (angles compared, angles
    excluded, of them orientation ties, bits compared, bits excluded)"""
    a_cmp = a_exc = a_tie = b_cmp = b_exc = 0
    for k, d in zip(kps32, desc32):
        lvl = int(k["class_id"])
        L = plan.lv[lvl]
        P = ref[lvl]
        r = float(2 ** L.octave)
        xf, yf = float(np.float32(k["x"]) / np.float32(r)), float(np.float32(k["y"]) / np.float32(r))
        s = int(np.floor(0.5 * float(k["size"]) / r + 0.5))
        ang, amb, tie = orientation(P["Lx"], P["Ly"], xf, yf, s)
        a_tie += int(tie)
        if amb:
            a_exc += 1
        else:
            diff = abs((float(k["angle"]) - ang + np.pi) % (2 * np.pi) - np.pi)
            assert diff <= BOUND_ANGLE, ("angle", lvl, float(k["x"]), float(k["y"]), float(k["angle"]), ang)
            a_cmp += 1
        mt, mg = float(np.max(np.abs(P["Lt"]))), max(float(np.max(np.abs(P["Lx"]))), float(np.max(np.abs(P["Ly"]))))
        eg = 2.0 * (max(BOUND_PLANE["Lx"], BOUND_PLANE["Ly"]) + BOUND_MLDB_SUM) * mg
        eps3 = [2.0 * (BOUND_PLANE["Lt"] + BOUND_MLDB_SUM) * mt, eg, eg]
        bits, sure = mldb_bits(mldb_values(P["Lt"], P["Lx"], P["Ly"], xf, yf, float(s), float(k["angle"])), eps3)
        got = np.unpackbits(np.asarray(d, np.uint8), bitorder="little")[:486].astype(bool)
        assert np.array_equal(got[sure], bits[sure]), ("mldb", lvl, float(k["x"]), float(k["y"]), np.nonzero(got[sure] != bits[sure])[0][:8])
        b_cmp += int(sure.sum()); b_exc += int((~sure).sum())
    return a_cmp, a_exc, a_tie, b_cmp, b_exc

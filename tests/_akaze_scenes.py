"""edge scenes for the AKAZE61 path (test data): frames that drive the oracle and the kernels into their rarely taken branches

  * border:    Gaussian blobs swept across the descriptor-border margin of is_out_of_bounds (oracle/akaze.c:288) on all four sides, at
               the blob scales that peak at octave 0 and at octave 1 (maxima one pixel outside the margin dropped, on it kept);
  * mirror:    band-limited texture whose right half is the mirror image of its left half.  The whole chain is exactly mirror
               symmetric (every filter adds its taps in pairs, a + b == b + a), so maxima on both sides of the axis have bit-equal
               responses.  No such pair comes close enough to meet in the duplicate suppression: mirror pairs are an odd number of
               columns apart, and two blobs 3 columns apart merge into one maximum at the levels whose radius exceeds 3 pixels;
  * flat:      constant 77, saturated 255 (hmax == 0 -> the 0.03 fallback of akz_kcontrast);
  * two_level: vertical stripes of 100 and 200 on 0.  Doubling the contrast doubles every float exactly, so the 100-edge's peak
               magnitude is exactly hmax / 2: those pixels sit exactly on the boundary of bin 150, and the 70th percentile lands among
               them; the 200-edge's peak is hmax itself and is folded from bin nbins into the last bin;
  * plateau:   isolated blobs on a constant background: the MLDB cells far from the blob sample exactly flat planes (constant Lt,
               zero derivatives), so their averages are bit-equal and the strict comparison gives 0 both ways;
  * symmetric: isotropic blobs centred on pixels, alone on a constant background: the orientation windows of the 0.15-rad sweep reach
               their maximum |sum|^2 in several windows with different samples, equal up to rounding (the float32 rounding decides).
tests/test_oracle_akaze_scenes.py proves on the oracle that each scene reaches its branch.
numpy only, no global RNG state: the same arguments give the same bytes."""
import numpy as np

W, H = 320, 240

# is_out_of_bounds keeps level pixel x iff fRound(x - 10 sqrt2 * S) - 1 >= 0 and fRound(x + 10 sqrt2 * S) + 1 < w: the first kept column
# per sigma_size S (and symmetrically w - 1 - MARGIN[S] the last one)
MARGIN = {2: 29, 3: 43, 4: 58}


def _blob(img, cx, cy, sigma, amp):
    h, w = img.shape
    r = int(np.ceil(4 * sigma))
    y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, h), max(cx - r, 0), min(cx + r + 1, w)
    yy, xx = np.mgrid[y0:y1, x0:x1]
    img[y0:y1, x0:x1] += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))


def border(w=W, h=H):
    """blobs of sigma 2.5 (peak at octave 0, S = 2) and 5 (octave 1) at distances MARGIN-3 .. MARGIN+3 from each side"""
    img = np.full((h, w), 60.0)
    for k, d in enumerate(range(MARGIN[2] - 3, MARGIN[2] + 4)):
        y = 40 + 24 * k
        _blob(img, d, y, 2.5, 150)                     # left
        _blob(img, w - 1 - d, y, 2.5, 150)             # right
        x = 60 + 30 * k
        _blob(img, x, d, 2.5, 150)                     # top
        _blob(img, x + 12, h - 1 - d, 2.5, 150)        # bottom
    for k, d in enumerate(range(2 * MARGIN[2] - 6, 2 * MARGIN[2] + 7, 3)):
        _blob(img, w // 2 - 80 + 32 * k, d, 5.0, 150)          # octave 1, top
        _blob(img, w // 2 - 64 + 32 * k, h - 1 - d, 5.0, 150)  # octave 1, bottom
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def mirror(w=W, h=H, seed=3):
    """band-limited noise, right half = mirror of the left half (w even: column x and w - 1 - x hold the same bytes)"""
    rng = np.random.default_rng(seed)
    k = np.exp(-0.5 * (np.arange(-6, 7) / 1.5) ** 2)
    k /= k.sum()
    a = rng.random((h + 12, w // 2 + 12))
    a = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 1, a)
    a = np.apply_along_axis(lambda c: np.convolve(c, k, "valid"), 0, a)
    a = (a - a.min()) / (a.max() - a.min())
    half = np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)
    return np.concatenate([half, half[:, ::-1]], 1)


def constant(w=W, h=H, v=77):
    return np.full((h, w), v, np.uint8)


TWO_LEVEL_STRIPES = ((60, 90, 100), (180, 210, 200))   # columns x0 .. x1 - 1 at the value, the rest 0


def two_level(w=W, h=H):
    img = np.zeros((h, w), np.uint8)
    for x0, x1, v in TWO_LEVEL_STRIPES:
        img[:, x0:x1] = v
    return img


def plateau(w=W, h=H):
    """a few blobs far apart on a constant 90: their descriptor cells away from the blob see exactly constant planes"""
    img = np.full((h, w), 90.0)
    for (x, y, s, a) in ((80, 80, 2.5, 120), (240, 80, 3.0, -70), (80, 170, 2.0, 140), (240, 170, 4.0, 110), (160, 125, 2.5, -80)):
        _blob(img, x, y, s, a)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def symmetric(w=W, h=H):
    """isotropic blobs centred on pixels, alone on a constant background (4-fold mirror symmetric samples around each)"""
    img = np.full((h, w), 40.0)
    for k, (x, y) in enumerate(((70, 70), (160, 70), (250, 70), (70, 170), (160, 170), (250, 170))):
        _blob(img, x, y, 2.0 + 0.5 * k, 160)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


SCENES = {"border": border, "mirror": mirror, "constant": constant, "saturated": lambda: constant(v=255), "two_level": two_level,
          "plateau": plateau, "symmetric": symmetric}
NAMES = list(SCENES)


def scene(name):
    return SCENES[name]()

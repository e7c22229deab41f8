"""Metamorphic-testing harness for the MUSICA pipeline — the counterpart of the reference's
test/metamorphic_test/script.py, restated on numpy/scipy and driving libmusica_hip.so.

The reference perturbs each raw image (collimator shutters, translations, rotations, Gaussian and
Poisson noise), runs `maverick-standalone <raw> <bmp>` and records three similarities between the
processed altered image and the processed unaltered image: 1 - RMSE/255 (`mse_similarity`,
script.py:143-145), SSIM (:147-152) and histogram distances (:154-198), both "direct" and
"registration based" (the altered result cropped / rotated back onto the unaltered one, :442-456,
:484-508, :586-608). It only logs the numbers. This module keeps the alteration generators, their
parameter grids and the metric definitions, can drive the library in-process or through the drop-in CLI
exactly like `run_process` (:200-214), and exposes the relations as data so tests can assert them on
phantoms (the reference's raw_images/ are missing blobs).
"""
import csv
import itertools
import math
import os
import subprocess

import numpy as np
from scipy import ndimage

from . import processing as mp

PROCESSING_MARGIN = 10  # script.py:24 == MUSICA_OUT_MARGIN

# alteration grids of the reference, for a 3072-pixel image (script.py:414, 459, 511, 562, 612, 636)
REF_IMAGE_SIZE = 3072
SHUTTERS = [200, 400, 600, 800, 1000]
TRANSLATIONS = [300, 600, 900, 1200, 1500]
ROTATIONS = [9, 18, 27, 36, 45]
GAUSS_SIGMAS = [4.0, 16.0, 64.0, 256.0, 1024.0]
POISSON_FACTORS = [0.1, 0.05, 0.025, 0.0125, 0.00625]
# not in the reference: the non-identity symmetries of the square (apply_symmetry), rows d4_<e> of a study run with `symmetries`
SYMMETRIES = (1, 2, 3, 4, 5, 6, 7)
# not in the reference: the radii of the resolution-loss rows (binomial_blur), rows blur_<r> of a study run with `blurs`
BLURS = (1, 2, 4, 8)


def scaled(values, image_size):
    """The reference's pixel-valued grids scaled from 3072 to `image_size`."""
    return [max(1, int(round(v * image_size / REF_IMAGE_SIZE))) for v in values]


# ---- alteration generators (script.py:49-141) ------------------------------------------------------

def apply_quantum_noise(image, scale_factor=1.0, rng=None):
    """script.py:49-58: Poisson noise at `scale_factor` of the dose."""
    rng = rng or np.random.default_rng()
    scaled_image = image.astype(np.float64) * scale_factor
    noisy = rng.poisson(scaled_image).astype(np.float32) / scale_factor
    return np.clip(noisy, 0, 65535).astype(np.uint16)


def add_gaussian_noise(image, mean, sigma, rng=None):
    """script.py:60-66: additive Gaussian noise, truncated to int before the add."""
    rng = rng or np.random.default_rng()
    noise = rng.normal(mean, sigma, image.shape).astype(np.int32)
    return np.clip(image.astype(np.int32) + noise, 0, 65535).astype(np.uint16)


def apply_collimator(image, shutter_h, shutter_v, rng=None):
    """script.py:75-95: outside the shutter rectangle the detector sees 1 % of the dose (+ Poisson noise)."""
    h, w = image.shape
    mask = np.zeros((h, w), dtype=bool)
    mask[shutter_v:h - shutter_v + 1, shutter_h:w - shutter_h + 1] = True   # PIL rectangles include both corners
    low = apply_quantum_noise((image / 100).astype(np.float64), 1, rng)
    return np.where(mask, image, low).astype(np.uint16)


def clamp_translation(image, x_shift, y_shift=0):
    """script.py:97-120: shift, filling the uncovered band with the 99th percentile of a 2-pixel strip."""
    h, w = image.shape
    bright, margin = 2, 10
    left = margin if x_shift > 0 else 0
    right = w - margin if x_shift < 0 else w
    top = margin if y_shift > 0 else 0
    bottom = h - margin if y_shift < 0 else h
    cropped = image[top:bottom, left:right]
    b_right = margin + bright if x_shift > 0 else w
    b_bottom = margin + bright if y_shift > 0 else h
    fill = int(np.percentile(image[top:b_bottom, left:b_right], 99))
    out = np.full((h, w), fill, dtype=np.uint16)
    ys, xs = max(y_shift, 0), max(x_shift, 0)
    hh, ww = min(cropped.shape[0], h - ys), min(cropped.shape[1], w - xs)
    out[ys:ys + hh, xs:xs + ww] = cropped[:hh, :ww]
    return out


def clamp_rotate(image, degree):
    """script.py:122-141: rotate the image minus a 100-pixel margin (nearest neighbour, counter-clockwise),
    filling with the 95th percentile."""
    h, w = image.shape
    margin = min(100, h // 8)
    cropped = image[margin:h - margin, margin:w - margin]
    fill = int(np.percentile(cropped, 95))
    rot = ndimage.rotate(cropped, degree, reshape=False, order=0, mode="constant", cval=fill)
    out = np.full((h, w), fill, dtype=np.uint16)
    out[margin:h - margin, margin:w - margin] = rot
    return out


def apply_symmetry(image, element):
    """Element 0 .. 7 of the symmetry group of the square (D4): np.rot90(x if element < 4 else x.T, element & 3). Output pixel (i, j) of
    a side-n plane is input pixel 0: [i, j], 1: [j, n-1-i], 2: [n-1-i, n-1-j], 3: [n-1-j, i], 4: [j, i] (transpose), 5: [n-1-i, j]
    (flipud), 6: [n-1-j, n-1-i] (anti-transpose), 7: [i, n-1-j] (fliplr): a permutation of the pixels, no fill and no resampling
    (not in the reference's script). Inverses: 1 <-> 3, every other element is its own."""
    element = int(element)
    if not 0 <= element <= 7:
        raise ValueError("symmetry element %d is not in 0 .. 7" % element)
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1]:
        raise ValueError("the symmetries of the square need a square image, got %r" % (image.shape,))
    return np.ascontiguousarray(np.rot90(image if element < 4 else image.T, element & 3))


def binomial_blur(image, radius):
    """The exact binomial blur of a 2-D uint16 or uint8 plane (not in the reference's script): resolution loss in integers. With
    r = radius in 1 .. BLUR_MAX_RADIUS and the weights w_k = C(2r, k), k = 0 .. 2r (their sum is 4^r),
        out[y, x] = (sum_i sum_j w_i w_j in[clamp(y + i - r), clamp(x + j - r)] + 2^(4r - 1)) >> 4r
    with indices clamped to the plane (edge replicated, no fill value). ONE rounding, after the full 2-D sum, halves rounded up; nothing
    is rounded between the two passes. The result has the input's dtype; a constant plane is preserved, so nothing saturates. The largest
    radius follows from the widths: the row pass of u16 data needs 16 + 2r <= 32 bits, the full sum 16 + 4r <= 48 (u64 here). At r = 8
    the blur is a Gaussian of sigma = sqrt(r / 2) = 2 pixels. This is the contract of musica_alter_blur and musica_sim_blur_reference
    (include/musica.h), which are bit-identical to it."""
    r = int(radius)
    if not 1 <= r <= mp.BLUR_MAX_RADIUS:
        raise ValueError("blur radius %d is not in 1 .. %d" % (r, mp.BLUR_MAX_RADIUS))
    image = np.asarray(image)
    if image.ndim != 2 or image.dtype not in (np.uint16, np.uint8) or not image.size:
        raise ValueError("binomial_blur needs a non-empty 2-D uint16 or uint8 plane, got %r %s" % (image.shape, image.dtype))
    acc = image.astype(np.uint64)
    for axis in (1, 0):           # rows, then columns: exact integers, so the order changes nothing
        padded = np.pad(acc, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode="edge")   # the clamped indices
        acc = np.zeros_like(acc)
        for k in range(2 * r + 1):
            acc += np.uint64(math.comb(2 * r, k)) * (padded[k:k + acc.shape[0]] if axis == 0 else padded[:, k:k + acc.shape[1]])
    return ((acc + np.uint64(1 << (4 * r - 1))) >> np.uint64(4 * r)).astype(image.dtype)


# ---- similarity metrics (script.py:143-198) ----------------------------------------------------------

def mse_similarity(a, b):
    """1 - RMSE / 255 (script.py:143-145)."""
    e = np.abs(a.astype(np.float64) - b.astype(np.float64)) / 255
    return 1.0 - math.sqrt(np.mean(np.square(e)))


def ssim_similarity(a, b):
    """skimage.metrics.structural_similarity with its defaults for uint8 input (script.py:147-152):
    7 x 7 uniform window, K1 = 0.01, K2 = 0.03, data range 255, sample covariance, borders cropped."""
    x, y = a.astype(np.float64), b.astype(np.float64)
    win = 7
    npx = win * win
    cov_norm = npx / (npx - 1)
    ux, uy = ndimage.uniform_filter(x, win), ndimage.uniform_filter(y, win)
    uxx, uyy, uxy = ndimage.uniform_filter(x * x, win), ndimage.uniform_filter(y * y, win), ndimage.uniform_filter(x * y, win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    pad = (win - 1) // 2
    return float(s[pad:-pad, pad:-pad].mean())


def hist_similarity(a, b):
    """(intersection, normalised Euclidean distance, Bhattacharyya coefficient) of the 256-bin histograms
    (script.py:154-198; np.histogram(bins=256) spans [min, max] of each image, as there)."""
    ha, _ = np.histogram(a.ravel(), bins=256)
    hb, _ = np.histogram(b.ravel(), bins=256)
    inter = np.sum(np.minimum(ha, hb)) / min(np.sum(ha), np.sum(hb))
    na, nb = ha / np.sum(ha), hb / np.sum(hb)
    e_dist = math.sqrt(np.sum((na - nb) ** 2)) / math.sqrt(2)
    b_coef = float(np.sum(np.sqrt(na * nb)))
    return float(inter), float(e_dist), b_coef


def similarities(a, b):
    inter, e_dist, b_coef = hist_similarity(a, b)
    return {"mse": mse_similarity(a, b), "ssim": ssim_similarity(a, b), "hist_intersection": inter,
            "hist_distance": e_dist, "hist_bhattacharyya": b_coef}


# ---- tone metrics from the joint gray-level histogram (not in the reference's script) ----------------------
# MUSICA's gradation follows the image's own histogram, so an alteration that changes the histogram moves the global tone curve of the
# output, and mse / ssim charge that shift in full. The joint histogram J[a][b] of two aligned 8-bit images separates it: mutual
# information (Viola & Wells; Maes et al.) and the correlation ratio (Roche et al.) do not change under an invertible remap of b's gray
# levels, and the least-squares remap E[a | b] itself turns a comparison into a tone-matched one. These functions state the numbers of
# musica_sim_joint (include/musica.h) in Python integers and f64, in its summation order.

def joint_histogram(a, b):
    """J[a][b]: how many pixels have the value a in `a` and b in `b` (two uint8 arrays of one shape); (256, 256) int64."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("joint_histogram needs two uint8 arrays of one shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    return np.bincount(a.ravel().astype(np.int64) * 256 + b.ravel(), minlength=65536).reshape(256, 256)


def _joint_moments(J):
    """Per value b of the second image, as Python integers: B_b (count), S_b = sum_a a J[a][b], Q_b = sum_a a^2 J[a][b]."""
    J = np.asarray(J).astype(np.int64)
    v = np.arange(256, dtype=np.int64)
    return [int(x) for x in J.sum(axis=0)], [int(x) for x in v @ J], [int(x) for x in (v * v) @ J]


def tone_lut(J):
    """The least-squares gray-level remap of b onto a, E[a | b] rounded half up: (2 S_b + B_b) // (2 B_b) where b occurs, else b;
    (256,) uint8."""
    B, S, _ = _joint_moments(J)
    return np.array([(2 * S[b] + B[b]) // (2 * B[b]) if B[b] else b for b in range(256)], dtype=np.uint8)


def joint_similarities(J):
    """mi, nmi, corr_ratio, tone_mse and the entropies h_a, h_b, h_ab (nats) of a joint histogram, as musica_sim_joint computes them:
    sums in ascending a, then ascending b, zero counts skipped; the variance numerators as exact integers, one f64 division per term."""
    J = np.asarray(J).astype(np.int64)
    n = int(J.sum())
    if n == 0:
        raise ValueError("empty joint histogram")
    A = [int(x) for x in J.sum(axis=1)]
    B, S, Q = _joint_moments(J)
    dn = float(n)

    def entropy(counts):
        h = 0.0
        for c in counts:
            if c:
                p = float(c) / dn
                h -= p * math.log(p)
        return h

    h_a, h_b = entropy(A), entropy(B)
    h_ab = mi = 0.0
    for a, b in zip(*np.nonzero(J)):          # row-major: ascending a, then ascending b
        j = int(J[a, b])
        p = float(j) / dn
        h_ab -= p * math.log(p)
        mi += p * math.log(float(j * n) / float(A[a] * B[b]))
    ssw = 0.0
    for b in range(256):
        if B[b]:
            ssw += float(B[b] * Q[b] - S[b] * S[b]) / float(B[b])
    sst_num = n * sum(a * a * A[a] for a in range(256)) - sum(a * A[a] for a in range(256)) ** 2
    return {"mi": mi, "nmi": 1.0 if h_a + h_b == 0.0 else 2.0 * mi / (h_a + h_b),
            "corr_ratio": 1.0 if sst_num == 0 else 1.0 - ssw / (float(sst_num) / dn),
            "tone_mse": 1.0 - math.sqrt(ssw / dn) / 255.0, "h_a": h_a, "h_b": h_b, "h_ab": h_ab}


def tone_similarities(a, b):
    """The five JOINT_METRICS of two uint8 images of one shape: mi (mutual information, nats), nmi (2 mi / (h_a + h_b)), corr_ratio
    (1 - SSW / SST: the share of a's variance a function of b explains), tone_mse (mse_similarity after the best gray-level remap of b
    onto a: 1 - sqrt(SSW / n) / 255) and tone_ssim (ssim_similarity of a and b remapped with tone_lut)."""
    J = joint_histogram(a, b)
    r = joint_similarities(J)
    out = {k: r[k] for k in mp.JOINT_METRICS if k != "tone_ssim"}
    out["tone_ssim"] = ssim_similarity(a, tone_lut(J)[b])
    return out


# ---- where the output went: exact block matching (musica_sim_displace; not in the reference) ------------------

def _displacement_geometry(a_shape, b_shape, region, radius):
    """Raises ValueError exactly where musica_sim_displace refuses a query on geometry; returns the region and radius as ints."""
    ax, ay, bx, by, w, h = (int(v) for v in region)
    radius = int(radius)
    if not 1 <= radius <= mp.SIM_MAX_RADIUS:
        raise ValueError("radius %d out of range [1, %d]" % (radius, mp.SIM_MAX_RADIUS))
    if w < 7 or h < 7:
        raise ValueError("region %d x %d is smaller than 7 x 7" % (w, h))
    if ax < 0 or ay < 0 or ax + w > a_shape[1] or ay + h > a_shape[0]:
        raise ValueError("region (%d, %d) + %d x %d leaves the %d x %d output plane" % (ax, ay, w, h, a_shape[1], a_shape[0]))
    if bx < radius or by < radius or bx + w + radius > b_shape[1] or by + h + radius > b_shape[0]:
        raise ValueError("the b window (%d, %d) + %d x %d grown by the radius %d leaves the %d x %d plane" % (bx, by, w, h, radius, b_shape[1], b_shape[0]))
    return (ax, ay, bx, by, w, h), radius


def _displacement_squares(a, b, region, radius):
    """((dy, dx), the h x w int64 squared differences of the region under that shift) for every candidate, one shifted crop each."""
    ax, ay, bx, by, w, h = region
    ca = np.asarray(a)[ay:ay + h, ax:ax + w].astype(np.int64)
    b = np.asarray(b)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            yield (dy, dx), (ca - b[by + dy:by + dy + h, bx + dx:bx + dx + w].astype(np.int64)) ** 2


def displacement_table(a, b, region, radius):
    """musica_sim_displace's table of one query, restated: a the output image, b the full reference plane, region = (ax, ay, bx, by, w, h).
    T[dy + radius][dx + radius] = sum over the region of (a[ay + y][ax + x] - b[by + y + dy][bx + x + dx])^2 for dy, dx in
    [-radius, radius], one shifted crop per candidate, in int64. ValueError where the C call refuses on geometry: a radius outside
    1 .. 16, w < 7 or h < 7, an a region that leaves a, a b window that, grown by the radius, leaves b."""
    region, radius = _displacement_geometry(np.shape(a), np.shape(b), region, radius)
    T = np.empty((2 * radius + 1,) * 2, dtype=np.int64)
    for (dy, dx), sq in _displacement_squares(a, b, region, radius):
        T[dy + radius, dx + radius] = np.sum(sq)
    return T


def displacement_tile_tables(a, b, region, radius):
    """The same per 64 x 64 tile of the region (the last tiles ragged): (tiles_y, tiles_x, S, S) uint32, tile-row major; their sum over
    the tiles is displacement_table."""
    region, radius = _displacement_geometry(np.shape(a), np.shape(b), region, radius)
    w, h = region[4], region[5]
    t = mp.SIM_TILE
    ny, nx, s = (h + t - 1) // t, (w + t - 1) // t, 2 * radius + 1
    out = np.empty((ny, nx, s, s), dtype=np.uint32)
    for (dy, dx), sq in _displacement_squares(a, b, region, radius):
        out[:, :, dy + radius, dx + radius] = np.add.reduceat(np.add.reduceat(sq, np.arange(0, h, t), axis=0), np.arange(0, w, t), axis=1)
    return out


def _displacement_argmin(T):
    """(row, column) of the table's argmin: smallest value, then smallest dx^2 + dy^2, then smallest dy, then smallest dx."""
    T = np.asarray(T)
    radius = T.shape[0] // 2
    ys, xs = np.nonzero(T == T.min())
    return min(zip(ys.tolist(), xs.tolist()), key=lambda p: ((p[1] - radius) ** 2 + (p[0] - radius) ** 2, p[0], p[1]))


def displacement_from_table(T):
    """{dx, dy, ssd_min, ssd_zero, sub_dx, sub_dy} of an (S, S) displacement table: the argmin by the tie rule, and the vertex of the
    parabola through the argmin and its two neighbours along the row (sub_dx) and along the column (sub_dy):
    sub = d + (T- - T+) / (2 (T- - 2 T0 + T+)), computed from the exact integers with one f64 division, where |d| < radius and the
    denominator is positive, else sub = d. The device and the host studies both call this on exact integer tables."""
    T = np.asarray(T)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or T.shape[0] % 2 != 1 or T.shape[0] < 3:
        raise ValueError("expected an (S, S) table with S = 2 radius + 1, got %r" % (T.shape,))
    radius = T.shape[0] // 2
    y, x = _displacement_argmin(T)

    def vertex(d, lo, mid, hi):
        if abs(d) >= radius:
            return float(d)
        lo, mid, hi = int(lo()), int(mid), int(hi())
        den = 2 * (lo - 2 * mid + hi)
        return d + (lo - hi) / den if den > 0 else float(d)

    dx, dy = x - radius, y - radius
    return {"dx": dx, "dy": dy, "ssd_min": int(T[y, x]), "ssd_zero": int(T[radius, radius]),
            "sub_dx": vertex(dx, lambda: T[y, x - 1], T[y, x], lambda: T[y, x + 1]),
            "sub_dy": vertex(dy, lambda: T[y - 1, x], T[y, x], lambda: T[y + 1, x])}


def displacement_tiles_off(tile_tables):
    """How many tiles' own argmin (the same tie rule) is not (0, 0)."""
    tt = np.asarray(tile_tables)
    radius = tt.shape[2] // 2
    return sum(1 for ty in range(tt.shape[0]) for tx in range(tt.shape[1]) if _displacement_argmin(tt[ty, tx]) != (radius, radius))


SHIFT_KEYS = ("dx", "dy", "sub_dx", "sub_dy", "mse_at_zero", "mse_at_best", "tiles", "tiles_off")


def displacement_summary(T, pixels, tiles, tiles_off):
    """A study row's *_shift dict (SHIFT_KEYS) from an exact table: displacement_from_table's shift, 1 - sqrt(ssd / pixels) / 255 at the
    zero shift and at the best one, the number of tiles and of those whose own best shift is not (0, 0)."""
    d = displacement_from_table(T)
    out = {k: d[k] for k in ("dx", "dy", "sub_dx", "sub_dy")}
    out["mse_at_zero"] = 1.0 - math.sqrt(d["ssd_zero"] / int(pixels)) / 255.0
    out["mse_at_best"] = 1.0 - math.sqrt(d["ssd_min"] / int(pixels)) / 255.0
    out["tiles"], out["tiles_off"] = int(tiles), int(tiles_off)
    return out


def displacement_maps(tile_tables, w, h):
    """Two (tiles_y, tiles_x) uint8 maps of a w x h region's tile tables, one pixel per tile: the RMSE at the zero shift, rounded, and the
    length of the tile's best shift, scaled so that the table's corner (radius, radius) is 255."""
    tt = np.asarray(tile_tables)
    ny, nx, radius, t = tt.shape[0], tt.shape[1], tt.shape[2] // 2, mp.SIM_TILE
    rmse, mag = np.zeros((ny, nx), dtype=np.uint8), np.zeros((ny, nx), dtype=np.uint8)
    for ty in range(ny):
        for tx in range(nx):
            px = (min(h, t * ty + t) - t * ty) * (min(w, t * tx + t) - t * tx)
            rmse[ty, tx] = int(round(math.sqrt(int(tt[ty, tx, radius, radius]) / px)))
            y, x = _displacement_argmin(tt[ty, tx])
            mag[ty, tx] = int(round(255.0 * math.hypot(x - radius, y - radius) / (math.sqrt(2.0) * radius)))
    return rmse, mag


def _inset(region, r):
    """The region (ax, ay, bx, by, w, h) inset by r on every side, or None when a side falls under 7."""
    ax, ay, bx, by, w, h = region
    return (ax + r, ay + r, bx + r, by + r, w - 2 * r, h - 2 * r) if min(w, h) - 2 * r >= 7 else None


# ---- at which scale the output changed: multi-scale SSIM in exact integers (musica_sim_multiscale; not in the reference) ----
# MUSICA is a Laplacian pyramid and each of its stages works at scales of its own (per-level contrast curves, noise reduction on levels
# 0 .. 2, the CNR weighting from level 3, the coarser-levels gain); a single 7 x 7 SSIM cannot tell a loss in the finest bands from a
# change of the coarse ones. Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) with ssim_similarity's uniform 7 x 7 window has an exact
# integer form: iterated 2 x 2 mean pooling is the 2^s x 2^s block mean, the block SUMS of u8 data are integers (<= 255 * 4^s), so every
# window sum at every scale is an exact integer and only the last f64 summation is open to reordering. These functions are the contract
# of musica_sim_multiscale (include/musica.h).
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # the 2003 paper's
SCALES_KEYS = ("ms_ssim", "scales") + mp.SCALE_METRICS        # a study row's *_scales dict


def block_sums(a, s):
    """X_s of a 2-D integer array: [i][j] = the sum of the 2^s x 2^s block whose top-left is (i 2^s, j 2^s); (h >> s, w >> s) int64,
    rows and columns that do not fill a block dropped."""
    a = np.asarray(a)
    k = 1 << s
    hs, ws = a.shape[0] >> s, a.shape[1] >> s
    return a[:hs * k, :ws * k].astype(np.int64).reshape(hs, k, ws, k).sum(axis=(1, 3))


def _window_sums7(p):
    """The sums of all 7 x 7 windows of an int64 plane, (h - 6, w - 6) int64: differences of its summed-area table (exact)."""
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(axis=0).cumsum(axis=1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def multiscale_terms(sx, sy, sxx, syy, sxy, s):
    """(ssim, cs, lum) per window from the exact 7 x 7 window sums of X_s, Y_s, X_s^2, Y_s^2, X_s Y_s (int64 arrays or ints): the means
    by one f64 division by the exact doubles 49 * 4^s and 49 * 16^s, then ssim_similarity's expression in its order."""
    d1, d2 = float(49 * 4 ** s), float(49 * 16 ** s)
    ux, uy = np.asarray(sx, dtype=np.int64) / d1, np.asarray(sy, dtype=np.int64) / d1
    uxx, uyy, uxy = np.asarray(sxx, dtype=np.int64) / d2, np.asarray(syy, dtype=np.int64) / d2, np.asarray(sxy, dtype=np.int64) / d2
    cov_norm = 49 / 48
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a1, a2, b1, b2 = 2 * ux * uy + c1, 2 * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2), a2 / b2, a1 / b1


def multiscale_windows(a, b, s):
    """(ssim, cs, lum), each (h_s - 6, w_s - 6) f64: the per-window values of scale s of two uint8 arrays of one shape."""
    x, y = block_sums(a, s), block_sums(b, s)
    return multiscale_terms(_window_sums7(x), _window_sums7(y), _window_sums7(x * x), _window_sums7(y * y), _window_sums7(x * y), s)


def ms_ssim_from_means(cs, ssim_last):
    """The combined number from the per-scale means: prod over s < scales - 1 of max(cs[s], 0)^w_s, times max(ssim of the last scale,
    0)^w_last, w_s = W[s] / sum(W[:scales]); math.pow, ascending s. cs: the means of scales 0 .. scales - 1 (the last is not used)."""
    n = len(cs)
    total = sum(MS_SSIM_WEIGHTS[:n])
    out = 1.0
    for s in range(n):
        out *= math.pow(max(float(cs[s]) if s < n - 1 else float(ssim_last), 0.0), MS_SSIM_WEIGHTS[s] / total)
    return out


def max_scales(w, h):
    """The largest scale count a w x h region admits: min(w, h) >> (count - 1) >= 7; 0 for a region under 7 x 7, at most SIM_MAX_SCALES."""
    n = 0
    while n < mp.SIM_MAX_SCALES and (min(int(w), int(h)) >> n) >= 7:
        n += 1
    return n


def multiscale_similarities(a, b, scales):
    """musica_sim_multiscale's numbers of two uint8 arrays of one shape (h, w), 1 <= scales <= 5, min(h, w) >> (scales - 1) >= 7 (else
    ValueError): {ms_ssim, scales, pixels, ssim, cs, lum, mse, ssd, plane_w, plane_h}, the last seven lists of length `scales`.
    ssim / cs / lum: the means of multiscale_windows over the windows; ssd[s] = sum (X_s - Y_s)^2 (exact);
    mse[s] = 1 - sqrt(ssd[s] / (h_s w_s)) / (255 * 4^s); ms_ssim: ms_ssim_from_means."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("multiscale_similarities needs two uint8 arrays of one 2-D shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    scales = int(scales)
    if not 1 <= scales <= mp.SIM_MAX_SCALES:
        raise ValueError("scales %d out of range [1, %d]" % (scales, mp.SIM_MAX_SCALES))
    h, w = a.shape
    if (min(h, w) >> (scales - 1)) < 7:
        raise ValueError("region %d x %d is smaller than the 7 x 7 window at scale %d" % (w, h, scales - 1))
    out = {"scales": scales, "pixels": h * w, "ssim": [], "cs": [], "lum": [], "mse": [], "ssd": [], "plane_w": [], "plane_h": []}
    for s in range(scales):
        ssim, cs, lum = multiscale_windows(a, b, s)
        hs, ws = h >> s, w >> s
        ssd = int(np.sum((block_sums(a, s) - block_sums(b, s)) ** 2))
        out["ssim"].append(float(ssim.mean()))
        out["cs"].append(float(cs.mean()))
        out["lum"].append(float(lum.mean()))
        out["ssd"].append(ssd)
        out["mse"].append(1.0 - math.sqrt(ssd / (hs * ws)) / (255 * 4 ** s))
        out["plane_w"].append(ws)
        out["plane_h"].append(hs)
    out["ms_ssim"] = ms_ssim_from_means(out["cs"], out["ssim"][-1])
    return out


# ---- bias and noise over many realisations: ensemble statistics (musica_sim_ensemble_*; not in the reference) ----
# A noise row scores ONE random draw, which cannot tell a systematic change of the output (a tone curve that moved with the gradation
# histogram, lost detail) from amplified noise, nor say how far the score moves under another seed. Over K realisations a_k of the same
# alteration the per-pixel sums S1 = sum a_k and S2 = sum a_k^2 give both: D = S1 - K b is K times the bias against the unaltered result
# b, V = K S2 - S1^2 is K (K - 1) times the sample variance. All of it is integer arithmetic; these functions are the contract of
# musica_sim_ensemble_result (include/musica.h).
ENSEMBLE_KEYS = mp.ENSEMBLE_METRICS + mp.ENSEMBLE_INTEGERS   # a study row's ensemble dicts; ensemble_statistics adds "tile_tables"


def ensemble_stream(ordinal, j):
    """The Philox stream of realisation j < 1024 of the study row with that ordinal (1, 2, ..): 1024 ordinal + j. Ordinals start at 1,
    so these streams never meet a row's own stream, its ordinal (a study has far fewer than 1024 rows)."""
    ordinal, j = int(ordinal), int(j)
    if ordinal < 1 or not 0 <= j < mp.SIM_ENSEMBLE_MAX:
        raise ValueError("ensemble_stream: ordinal %d must be >= 1 and the realisation %d in 0 .. %d" % (ordinal, j, mp.SIM_ENSEMBLE_MAX - 1))
    return mp.SIM_ENSEMBLE_MAX * ordinal + j


def ensemble_summary(sq_bias_sum, var_sum, sq_err_sum, bias_sum, abs_bias_max, var_max, realisations, w, h):
    """A query's ENSEMBLE_KEYS dict from its exact integers: the doubles one IEEE operation each in include/musica.h's order, every
    integer converted to double first. The device and the host studies both call this, so they agree to the last bit."""
    ints = [int(v) for v in (sq_bias_sum, var_sum, sq_err_sum, bias_sum, abs_bias_max, var_max)]
    k, n = int(realisations), int(w) * int(h)
    sq_bias, var, sq_err, bias = ints[:4]
    if k * sq_err != sq_bias + var:
        raise ValueError("ensemble_summary: K sq_err_sum != sq_bias_sum + var_sum (%d * %d, %d + %d)" % (k, sq_err, sq_bias, var))
    t = mp.SIM_TILE
    out = {"mean_shift": float(bias) / float(k * n),
           "bias_rms": math.sqrt(float(sq_bias) / float(k * k * n)),
           "noise_rms": 0.0 if k == 1 else math.sqrt(float(var) / float(k * (k - 1) * n)),
           "mse": 1.0 - math.sqrt(float(sq_err) / float(k * n)) / 255.0,
           "bias_fraction": 0.0 if sq_bias + var == 0 else float(sq_bias) / float(sq_bias + var)}
    out.update(zip(mp.ENSEMBLE_INTEGERS, ints + [n, k, (int(w) + t - 1) // t, (int(h) + t - 1) // t]))
    return out


def ensemble_statistics(outs, b, region):
    """musica_sim_ensemble_result's numbers of one query, restated: outs a (K, H, W) stack of uint8 outputs (the realisations), b the full
    uint8 reference plane, region = (ax, ay, bx, by, w, h). Integer dtype throughout: S1, S2, D, V and the error term per pixel and the
    tile sums in int64 (a tile's sum D^2 <= 64^2 * 261120^2 < 2^63), the totals as Python ints summed over the tiles. Returns the
    ENSEMBLE_KEYS dict (ensemble_summary) plus "tile_tables": (tiles_y, tiles_x, 2) uint64, (sum D^2, sum V) per 64 x 64 tile. ValueError
    where the C call refuses: no or more than SIM_ENSEMBLE_MAX realisations, w < 7 or h < 7, a region that leaves either plane,
    65025 K^2 w h >= 2^64."""
    outs, b = np.asarray(outs), np.asarray(b)
    if outs.ndim != 3 or b.ndim != 2 or outs.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("ensemble_statistics needs a (K, H, W) uint8 stack and a 2-D uint8 plane, got %r %s and %r %s" % (outs.shape, outs.dtype, b.shape, b.dtype))
    k = outs.shape[0]
    if not 1 <= k <= mp.SIM_ENSEMBLE_MAX:
        raise ValueError("%d realisations out of range [1, %d]" % (k, mp.SIM_ENSEMBLE_MAX))
    ax, ay, bx, by, w, h = (int(v) for v in region)
    if w < 7 or h < 7:
        raise ValueError("region %d x %d is smaller than 7 x 7" % (w, h))
    if min(ax, ay, bx, by) < 0 or ax + w > outs.shape[2] or ay + h > outs.shape[1] or bx + w > b.shape[1] or by + h > b.shape[0]:
        raise ValueError("region (%d, %d) / (%d, %d) + %d x %d leaves the planes" % (ax, ay, bx, by, w, h))
    if 65025 * k * k * w * h >= 2 ** 64:
        raise ValueError("65025 * %d^2 * %d * %d does not fit 64 bits" % (k, w, h))
    a = outs[:, ay:ay + h, ax:ax + w].astype(np.int64)
    cb = b[by:by + h, bx:bx + w].astype(np.int64)
    s1, s2 = a.sum(axis=0), (a * a).sum(axis=0)
    d = s1 - k * cb
    v = k * s2 - s1 * s1
    e = s2 - 2 * cb * s1 + k * cb * cb
    t = mp.SIM_TILE

    def tiles(x):
        return np.add.reduceat(np.add.reduceat(x, np.arange(0, h, t), axis=0), np.arange(0, w, t), axis=1)

    tile_tables = np.stack([tiles(d * d), tiles(v)], axis=-1).astype(np.uint64)
    out = ensemble_summary(sum(int(x) for x in tile_tables[..., 0].ravel()), sum(int(x) for x in tile_tables[..., 1].ravel()),
                           sum(int(x) for x in tiles(e).ravel()), sum(int(x) for x in tiles(d).ravel()), int(np.abs(d).max()), int(v.max()), k, w, h)
    out["tile_tables"] = tile_tables
    return out


def ensemble_maps(tile_tables, w, h, realisations):
    """Two (tiles_y, tiles_x) uint8 maps of a w x h region's ensemble tile table, one pixel per tile: the tile's bias rms,
    sqrt(sum D^2 / (K^2 pixels)), and its noise rms, sqrt(sum V / (K (K - 1) pixels)) (0 for K == 1), in gray levels, rounded."""
    tt = np.asarray(tile_tables)
    ny, nx, t, k = tt.shape[0], tt.shape[1], mp.SIM_TILE, int(realisations)
    bias, noise = np.zeros((ny, nx), dtype=np.uint8), np.zeros((ny, nx), dtype=np.uint8)
    for ty in range(ny):
        for tx in range(nx):
            px = (min(h, t * ty + t) - t * ty) * (min(w, t * tx + t) - t * tx)
            bias[ty, tx] = min(255, int(round(math.sqrt(int(tt[ty, tx, 0]) / (k * k * px)))))
            noise[ty, tx] = min(255, int(round(math.sqrt(int(tt[ty, tx, 1]) / (k * (k - 1) * px))))) if k > 1 else 0
    return bias, noise


# ---- the texture of the noise: spatial auto-covariance and power spectrum (musica_sim_ensemble_track / _covariance; not in the reference) ----
# The per-pixel statistics say how strong the output noise is and nothing about its grain: MUSICA amplifies fine pyramid levels more than
# coarse ones and its noise reduction works on 5 x 5 neighbourhoods, so the noise that leaves it is coloured. Over K realisations a_k,
# with S1 = sum_k a_k, the lag products P(d) = sum_k sum_p a_k(p) a_k(p + d) and U(d) = sum_p S1(p) S1(p + d) over a region of n pixels
# give C(d) = K P(d) - U(d) = K^2 n times the population covariance at lag d about the per-pixel ensemble mean, in exact integers; the
# neighbour correlations, the correlation area and the noise power spectrum (Wiener-Khinchin) follow. These functions are the contract
# of musica_sim_ensemble_covariance (include/musica.h).
COV_KEYS = mp.COV_METRICS + mp.COV_INTEGERS   # ensemble_covariance adds "table" and "tile_tables"; a study row's dicts add "nps_radial" and "hf_fraction"


def _covariance_geometry(shape, region, radius):
    """Raises ValueError exactly where musica_sim_ensemble_track refuses a region on geometry; returns (ax, ay, w, h) and the radius as
    ints. region: (ax, ay, w, h), or a query's (ax, ay, bx, by, w, h), whose bx, by only have to stay inside the plane."""
    region = tuple(int(v) for v in region)
    if len(region) == 6:
        ax, ay, bx, by, w, h = region
    else:
        ax, ay, w, h = region
        bx, by = ax, ay
    radius = int(radius)
    if not 1 <= radius <= mp.SIM_MAX_RADIUS:
        raise ValueError("radius %d out of range [1, %d]" % (radius, mp.SIM_MAX_RADIUS))
    if w < 7 or h < 7:
        raise ValueError("region %d x %d is smaller than 7 x 7" % (w, h))
    if min(ax, ay, bx, by) < 0 or max(ax, bx) + w > shape[1] or max(ay, by) + h > shape[0]:
        raise ValueError("region (%d, %d) / (%d, %d) + %d x %d leaves the %d x %d plane" % (ax, ay, bx, by, w, h, shape[1], shape[0]))
    if ax < radius or ax + w + radius > shape[1] or ay + h + radius > shape[0]:
        raise ValueError("the window (%d, %d) + %d x %d grown by the radius %d (left, right, down) leaves the %d x %d plane" % (ax, ay, w, h, radius, shape[1], shape[0]))
    if 65025 * mp.SIM_ENSEMBLE_MAX ** 2 * w * h >= 2 ** 63:
        raise ValueError("65025 * %d^2 * %d * %d does not fit 63 bits" % (mp.SIM_ENSEMBLE_MAX, w, h))
    return (ax, ay, w, h), radius


def covariance_summary(table, realisations, pixels):
    """The doubles of a covariance result from its exact (R + 1, 2 R + 1) table C(d) (row dy, column dx + R), one IEEE operation each in
    include/musica.h's order, every integer converted to double first, with c00, pixels, realisations and radius. The device and the
    host studies both call this, so they agree to the last bit."""
    table = np.asarray(table)
    if table.ndim != 2 or table.shape[0] < 2 or table.shape[1] != 2 * table.shape[0] - 1:
        raise ValueError("expected an (R + 1, 2 R + 1) table, got %r" % (table.shape,))
    r, k, n = table.shape[0] - 1, int(realisations), int(pixels)
    c00 = int(table[0, r])
    half = 0.0
    for dy in range(r + 1):
        for dx in range(-r if dy else 1, r + 1):
            half += float(int(table[dy, dx + r]))
    return {"noise_var": 0.0 if k == 1 else float(c00) / float(k * (k - 1) * n),
            "rho_x": 0.0 if c00 == 0 else float(int(table[0, r + 1])) / float(c00),
            "rho_y": 0.0 if c00 == 0 else float(int(table[1, r])) / float(c00),
            "corr_area": 1.0 if c00 == 0 else (float(c00) + 2.0 * half) / float(c00),
            "c00": c00, "pixels": n, "realisations": k, "radius": r}


def ensemble_covariance(outs, region, radius):
    """musica_sim_ensemble_covariance's numbers of one tracked region, restated: outs a (K, H, W) stack of uint8 outputs (the
    realisations), region = (ax, ay, w, h) or a query's (ax, ay, bx, by, w, h). For dy = 0 .. R and dx = -R .. R, per region pixel in
    int64, K sum_k a_k(p) a_k(p + d) - S1(p) S1(p + d), summed per 64 x 64 tile of the region (int64: a tile's |C| <= 4096 * 65025 K^2 <
    2^58), the region's totals as Python ints over the tiles. Returns the COV_KEYS dict (covariance_summary) plus "table":
    (R + 1, 2 R + 1) int64, row dy, column dx + R, and "tile_tables": (tiles_y, tiles_x, R + 1, 2 R + 1) int64. ValueError where the C
    calls refuse: no or more than SIM_ENSEMBLE_MAX realisations, a radius outside 1 .. 16, w < 7 or h < 7, a region that leaves the
    plane, a window that, grown by the radius to the left, to the right and downwards, leaves it, 65025 * 1024^2 w h >= 2^63."""
    outs = np.asarray(outs)
    if outs.ndim != 3 or outs.dtype != np.uint8:
        raise ValueError("ensemble_covariance needs a (K, H, W) uint8 stack, got %r %s" % (outs.shape, outs.dtype))
    k = outs.shape[0]
    if not 1 <= k <= mp.SIM_ENSEMBLE_MAX:
        raise ValueError("%d realisations out of range [1, %d]" % (k, mp.SIM_ENSEMBLE_MAX))
    (ax, ay, w, h), r = _covariance_geometry(outs.shape[1:], region, radius)
    t, s = mp.SIM_TILE, 2 * r + 1
    ny, nx = (h + t - 1) // t, (w + t - 1) // t
    a = outs.astype(np.int64)
    s1 = a.sum(axis=0)
    ca, c1 = a[:, ay:ay + h, ax:ax + w], s1[ay:ay + h, ax:ax + w]
    tile_tables = np.empty((ny, nx, r + 1, s), dtype=np.int64)
    for dy in range(r + 1):
        for dx in range(-r, r + 1):
            shifted = (slice(ay + dy, ay + dy + h), slice(ax + dx, ax + dx + w))
            c = k * (ca * a[(slice(None),) + shifted]).sum(axis=0) - c1 * s1[shifted]
            tile_tables[:, :, dy, dx + r] = np.add.reduceat(np.add.reduceat(c, np.arange(0, h, t), axis=0), np.arange(0, w, t), axis=1)
    table = np.array([[sum(int(x) for x in tile_tables[:, :, dy, j].ravel()) for j in range(s)] for dy in range(r + 1)], dtype=np.int64)
    out = covariance_summary(table, k, w * h)
    out.update(tiles_x=nx, tiles_y=ny, table=table, tile_tables=tile_tables)
    return out


def covariance_symmetric(table):
    """The (S, S) float64 table over dy, dx = -R .. R (row dy + R, column dx + R) of a half-plane table: C(-d) = C(d), the row dy = 0
    taken from its entries with dx >= 0."""
    table = np.asarray(table)
    r = table.shape[0] - 1
    sym = np.empty((2 * r + 1,) * 2, dtype=np.float64)
    sym[r + 1:] = table[1:]
    sym[:r] = table[1:][::-1, ::-1]
    sym[r, r:] = table[0, r:]
    sym[r, :r] = table[0, r + 1:][::-1]
    return sym


def noise_power_spectrum(table, realisations, pixels):
    """The noise power spectrum of a covariance table (Wiener-Khinchin), host only: N[v][u] = sum over d of C_sym(d)
    cos(2 pi (u dx + v dy) / S) / (K (K - 1) n) for u, v = 0 .. S - 1, (S, S) float64, the zero frequency at [0][0]. The sum of
    cosines is taken as cos cos - sin sin with the phases' integers reduced mod S first. All zero when K == 1."""
    sym = covariance_symmetric(table)
    s, k, n = sym.shape[0], int(realisations), int(pixels)
    if k == 1:
        return np.zeros((s, s), dtype=np.float64)
    d = np.arange(s) - s // 2
    phase = 2.0 * np.pi * ((np.arange(s)[:, None] * d[None, :]) % s) / s     # [frequency][lag]
    co, si = np.cos(phase), np.sin(phase)
    return (co @ sym @ co.T - si @ sym @ si.T) / float(k * (k - 1) * n)


def _nps_radius(s):
    d = np.arange(s) - s // 2
    return np.hypot(d[:, None], d[None, :])


def nps_radial(nps):
    """The mean of the centred spectrum (np.fft.fftshift) over the frequencies of rounded integer radius 0 .. R: a list of R + 1 floats."""
    nps = np.asarray(nps, dtype=np.float64)
    rad = np.rint(_nps_radius(nps.shape[0])).astype(np.int64)
    c = np.fft.fftshift(nps)
    return [float(c[rad == i].mean()) for i in range(nps.shape[0] // 2 + 1)]


def nps_hf_fraction(nps):
    """The share of the spectrum's sum at radius > R / 2 of the centred spectrum (0 for a spectrum that sums to 0). White noise gives
    the share of such frequencies among the S^2: nps_hf_fraction(np.ones((S, S)))."""
    nps = np.asarray(nps, dtype=np.float64)
    total = float(nps.sum())
    if total == 0.0:
        return 0.0
    return float(np.fft.fftshift(nps)[_nps_radius(nps.shape[0]) > (nps.shape[0] // 2) / 2.0].sum()) / total


hf_fraction = nps_hf_fraction


def covariance_row(table, realisations, w, h):
    """A study row's covariance dict of one region from its exact table: COV_KEYS, then "nps_radial" and "hf_fraction"."""
    t = mp.SIM_TILE
    d = covariance_summary(table, realisations, int(w) * int(h))
    d.update(tiles_x=(int(w) + t - 1) // t, tiles_y=(int(h) + t - 1) // t)
    out = {k: d[k] for k in COV_KEYS}
    nps = noise_power_spectrum(table, realisations, int(w) * int(h))
    out["nps_radial"], out["hf_fraction"] = nps_radial(nps), nps_hf_fraction(nps)
    return out


def nps_map(table, realisations, pixels):
    """The centred spectrum as an (S, S) uint8 image: log(1 + max(N, 0)) scaled so that its largest value is 255, rounded."""
    v = np.log1p(np.maximum(np.fft.fftshift(noise_power_spectrum(table, realisations, pixels)), 0.0))
    top = float(v.max())
    return np.zeros(v.shape, dtype=np.uint8) if top == 0.0 else np.rint(255.0 * v / top).astype(np.uint8)


# ---- the vendor-processed reference image (script.py:395-411) ------------------------------------------

def vendor_to_u8(pixels):
    """The 8-bit image the reference compares against, from the vendor image's stored values (dicom.read_dicom_gray): for 16-bit data
    Image.point(i * 1/256).convert('L') truncates to v >> 8, and ImageOps.invert is 255 - v, whatever the DICOM's
    PhotometricInterpretation says. So 255 - (v >> 8) for uint16, 255 - v for uint8 (checked against Pillow for every value)."""
    a = np.asarray(pixels)
    if a.dtype == np.uint16:
        return (255 - (a >> 8)).astype(np.uint8)
    if a.dtype == np.uint8:
        return 255 - a
    raise ValueError("vendor image must be uint8 or uint16, got %s" % a.dtype)


# ---- registration of the altered result onto the unaltered one (script.py:442-456, 484-508, 586-608) ----
# The geometry lives in the *_rects functions: one rectangle (x, y, w, h) per side, exactly what the reference's slices select (Python's
# clamping of slice bounds included). register_* slice with them; roi_* state them as the (ax, ay, bx, by, w, h) region of a device-side
# comparison (musica_sim_compare), or None when the two slices differ in shape (the study then has no registered comparison).

def _span(start, stop, n):
    """What a[start:stop] selects along an axis of length n: (first index, length)."""
    first, end, _ = slice(start, stop).indices(n)
    return first, max(0, end - first)


def _rect(shape, y0, y1, x0, x1):
    y, h = _span(y0, y1, shape[0])
    x, w = _span(x0, x1, shape[1])
    return x, y, w, h


def _crop(alt, unalt, rects):
    (ax, ay, aw, ah), (bx, by, bw, bh) = rects
    return alt[ay:ay + ah, ax:ax + aw], unalt[by:by + bh, bx:bx + bw]


def _roi(rects):
    (ax, ay, aw, ah), (bx, by, bw, bh) = rects
    return (ax, ay, bx, by, aw, ah) if (aw, ah) == (bw, bh) else None


def collimator_rects(a_shape, b_shape, shutter):
    x = y = shutter + PROCESSING_MARGIN
    w = a_shape[1] - (2 * shutter + 2 * PROCESSING_MARGIN)
    h = a_shape[0] - (2 * shutter + 2 * PROCESSING_MARGIN)
    return _rect(a_shape, y, y + h, x, x + w), _rect(b_shape, y, y + h, x, x + w)


def translation_x_rects(a_shape, b_shape, tx):
    return _rect(a_shape, None, None, tx, None), _rect(b_shape, None, None, PROCESSING_MARGIN, a_shape[1] - tx + PROCESSING_MARGIN)


def translation_y_rects(a_shape, b_shape, ty):
    return _rect(a_shape, ty, None, None, None), _rect(b_shape, PROCESSING_MARGIN, a_shape[0] - ty + PROCESSING_MARGIN, None, None)


def rotation_rects(a_shape, b_shape, degree):
    h, w = b_shape
    ang = math.radians(degree)
    new_w = w * abs(math.cos(ang)) + h * abs(math.sin(ang))
    new_h = h * abs(math.cos(ang)) + w * abs(math.sin(ang))
    inner_w = w * h / new_h if w < h else h * w / new_w
    inner_h = h * w / new_w if w < h else w * h / new_h
    left, top = int((w - inner_w) / 2), int((h - inner_h) / 2)
    right, bottom = int((w + inner_w) / 2), int((h + inner_h) / 2)
    return _rect(a_shape, top, bottom, left, right), _rect(b_shape, top, bottom, left, right)


def roi_collimator(shape, shutter, b_shape=None):
    return _roi(collimator_rects(shape, b_shape or shape, shutter))


def roi_translation_x(shape, tx, b_shape=None):
    return _roi(translation_x_rects(shape, b_shape or shape, tx))


def roi_translation_y(shape, ty, b_shape=None):
    return _roi(translation_y_rects(shape, b_shape or shape, ty))


def roi_rotation(shape, degree, b_shape=None):
    return _roi(rotation_rects(shape, b_shape or shape, degree))


def register_collimator(alt, unalt, shutter):
    return _crop(alt, unalt, collimator_rects(alt.shape, unalt.shape, shutter))


def register_translation_x(alt, unalt, tx):
    return _crop(alt, unalt, translation_x_rects(alt.shape, unalt.shape, tx))


def register_translation_y(alt, unalt, ty):
    return _crop(alt, unalt, translation_y_rects(alt.shape, unalt.shape, ty))


def rotated_reference(unalt, degree):
    """The unaltered result rotated like the alteration (nearest neighbour, zero fill), what register_rotation compares against."""
    return ndimage.rotate(unalt, degree, reshape=False, order=0, mode="constant", cval=0)


def register_rotation(alt, unalt, degree):
    return _crop(alt, rotated_reference(unalt, degree), rotation_rects(alt.shape, unalt.shape, degree))


def register_symmetry(alt, unalt, element):
    """The whole altered result against the unaltered result transformed like the alteration: the margin is symmetric, so nothing is cropped."""
    return alt, apply_symmetry(unalt, element)


def roi_symmetry(shape):
    """The full frame, as the region of a device-side comparison."""
    return (0, 0, 0, 0, shape[1], shape[0])


def register_blur(alt, unalt, radius):
    """The altered result against the unaltered result blurred like the alteration, both inset by the radius: within `radius` pixels of
    the output plane's border the blurred reference is built from clamped neighbours, while the altered output there came from real
    neighbours in the processing margin."""
    r = int(radius)
    h, w = alt.shape
    return alt[r:max(h - r, r), r:max(w - r, r)], binomial_blur(unalt, r)[r:max(h - r, r), r:max(w - r, r)]


def roi_blur(shape, radius):
    """The full frame inset by the radius, as the region of a device-side comparison; None when a side falls under 7."""
    return _inset((0, 0, 0, 0, shape[1], shape[0]), int(radius))


# ---- running the pipeline -------------------------------------------------------------------------

class Runner:
    """Processes raw images to the 8-bit output the reference's saveOutImage writes (margin cropped)."""

    def __init__(self, image_size, levels=0, device=0, use_cli=False, device_metrics=False, device_alterations=False, ensemble_batch=8):
        if use_cli and device_alterations:
            raise ValueError("device alterations write the library's resident input buffer: the CLI path has none")
        if use_cli and device_metrics:
            raise ValueError("device metrics score the library's device output: the CLI path has none")
        self.n, self.levels, self.device, self.use_cli = image_size, levels, device, use_cli
        self.device_alterations = device_alterations   # run_study generates the alterations on the device (musica_alter); implies device_metrics
        self.device_metrics = device_metrics or device_alterations   # run_study scores on the device (musica_sim_compare) instead of with numpy
        self.ensemble_batch = int(ensemble_batch)       # images per step of the ensemble context (run_study's ensemble=K)
        if self.ensemble_batch < 1:
            raise ValueError("ensemble_batch %d must be at least 1" % self.ensemble_batch)
        self.ensemble_proc = None                       # a second context of the runner's size, levels and device, created on first use
        self.proc = None
        if not use_cli:
            self.proc = mp.MusicaProcessing(device=device)
            if not self.proc.init(image_size, levels=levels):
                raise RuntimeError("musica_create failed: " + mp.last_error())

    def run(self, raw, workdir=None):
        """raw: (N, N) uint16 -> (N-20, N-20) uint8."""
        if self.use_cli:
            return self._run_cli(raw, workdir or ".")
        if not self.proc.execute(raw):
            raise RuntimeError("musica_execute failed: " + mp.last_error())
        return self.proc.out_pixels()

    def run_device(self, raw):
        """The same step, its output left on the device (for sim_capture / sim_compare)."""
        if not self.proc.execute(raw):
            raise RuntimeError("musica_execute failed: " + mp.last_error())

    def run_resident(self):
        """The step on the resident input buffer (what an alter_* call wrote), its output left on the device."""
        if not self.proc.execute_device():
            raise RuntimeError("musica_execute_device failed: " + mp.last_error())
        self.proc.sync()

    def mean_cnr(self):
        """mean(cnr image) * 256 of the last run — what test/mean_cnr/script.py prints for a cnr.bmp dump."""
        return self.proc.stats().mean_cnr

    def _run_cli(self, raw, workdir):
        """run_process of script.py:200-214: write the raw file, spawn the CLI, read the BMP back."""
        from .phantom import write_raw
        raw_path, out_path = os.path.join(workdir, "in.raw"), os.path.join(workdir, "out.bmp")
        write_raw(raw_path, raw)
        cmd = [mp.CLI_PATH, os.path.abspath(raw_path), os.path.abspath(out_path), "--size", str(self.n), "--device", str(self.device)]
        if self.levels:
            cmd += ["--levels", str(self.levels)]
        subprocess.run(cmd, check=True, capture_output=True)
        return read_bmp_gray(out_path)

    def ensemble_context(self, realisations):
        """The batch context run_study's ensembles run on, created on first use with a batch of min(ensemble_batch, realisations)."""
        if self.ensemble_proc is None:
            proc = mp.MusicaProcessing(device=self.device)
            if not proc.init(self.n, levels=self.levels, batch=max(1, min(self.ensemble_batch, int(realisations)))):
                raise RuntimeError("musica_create failed: " + mp.last_error())
            self.ensemble_proc = proc
        return self.ensemble_proc

    def close(self):
        if self.proc:
            self.proc.cleanup()
        if self.ensemble_proc:
            self.ensemble_proc.cleanup()
            self.ensemble_proc = None


def read_bmp_gray(path):
    """Reads the 24-bpp bottom-up BMP saveOutImage writes; returns the gray channel top-down."""
    b = open(path, "rb").read()
    off = int.from_bytes(b[10:14], "little")
    w, h = int.from_bytes(b[18:22], "little"), int.from_bytes(b[22:26], "little")
    row = (w * 3 + 3) & ~3
    a = np.frombuffer(b, dtype=np.uint8, count=row * h, offset=off).reshape(h, row)[:, 0:w * 3:3]
    return a[::-1].copy()


# reference slots of a device study: the unaltered result, it rotated, the vendor image, it rotated (VENDOR_SLOT: the vendor slot that
# stands beside an unaltered one)
SLOT_UNALTERED, SLOT_ROTATED, SLOT_VENDOR, SLOT_VENDOR_ROTATED = 0, 1, 2, 3
VENDOR_SLOT = {SLOT_UNALTERED: SLOT_VENDOR, SLOT_ROTATED: SLOT_VENDOR_ROTATED}
SLOT_TONE = 4   # tone=True: slots 4 .. 7 hold the slots of a row's (at most four) comparisons remapped with their tone_lut (musica_sim_remap_reference)
SCALE_ROW_KEYS = {"direct": "direct_scales", "registered": "registered_scales", "reference": "reference_scales",
                  "registered_reference": "registered_reference_scales"}
TONE_KEYS = {"direct": "direct_tone", "registered": "registered_tone", "reference": "reference_tone",
             "registered_reference": "registered_reference_tone"}


def run_study(raw, runner, rng=None, shutters=None, translations=None, rotations=None, sigmas=None, factors=None, vendor=None, symmetries=None,
              tone=False, displacement=0, displacement_tiles=False, scales=0, ensemble=0, ensemble_tiles=False, covariance=0, covariance_tiles=False,
              blurs=None):
    """The reference's per-image loop (script.py:383-657): returns a list of rows
    {alteration, direct: {...}, registered: {...} or None, mean_cnr}. With runner.device_metrics the similarities are computed
    on the device against the unaltered result kept in reference slot 0 (rotations: the rotated unaltered result in slot 1).

    With runner.device_alterations the raw image is uploaded once and every alteration is generated on the device (musica_alter),
    the rotated unaltered result comes from musica_sim_rotate_reference, and the seed of the noise alterations is drawn from `rng`, their
    ordinal in the study being the stream. The geometric alterations are bit-identical to the host's, so their rows equal a device-metrics
    study's; the noise rows (c_sh_*, gn_*, pn_*) come from a different, reproducible, stream than the host study's numpy draws.

    vendor: the vendor-processed image of `raw` ((N - 20, N - 20) uint8 or uint16, as dicom.read_dicom_gray returns it), compared as
    vendor_to_u8 converts it. Row 0 then gains "reference" (the unaltered result vs the vendor image: the reference's m_sim_ovd), every
    other row "reference" (the altered result vs the vendor image) and "registered_reference" (the registered crop vs the same crop of
    the vendor image, rotations: of the vendor image rotated as rotated_reference rotates; None exactly where "registered" is None).
    On the device the vendor image sits in slot 2 (musica_sim_set_vendor_reference), rotated in slot 3, and its queries join the
    row's own launch. Without it the rows are exactly as before.

    symmetries: elements of the square's symmetry group (apply_symmetry; SYMMETRIES for the seven non-trivial ones). None or empty adds
    nothing. Otherwise rows d4_<e> follow the pn_* rows: the raw image under element e (on the device: alter_symmetry), "direct" against
    the unaltered result, "registered" over the WHOLE frame against the unaltered result under the same element, which an exactly
    equivariant pipeline would reproduce bit for bit. On the device that reference goes into slot 1 and the transformed vendor image into
    slot 3 (musica_sim_transform_reference; the rotation rows are done with them by then). These rows draw nothing from `rng` and do not
    advance the noise ordinal.

    tone: every comparison dict of a row gains a sibling with the five JOINT_METRICS (tone_similarities): direct_tone, registered_tone
    and, with a vendor image, reference_tone and registered_reference_tone; present exactly where the original is and None exactly
    where it is None. On the device the row's queries go through musica_sim_joint in one call, each comparison's tone_lut remaps its
    slot into one of the slots SLOT_TONE .. SLOT_TONE + 3 (musica_sim_remap_reference), and tone_ssim is musica_sim_compare's ssim
    against those slots over the same regions, one call per row. Without it the rows and the launches are exactly as before.

    displacement: a radius R > 0 measures where the output went by exact block matching (displacement_table). Every row gains
    "direct_shift": the full frame inset by R on every side against the unaltered result; rows with a registered comparison gain
    "registered_shift": that comparison's region inset by R against what it is compared with (None exactly where "registered" is None or
    the inset region has a side under 7). Each is a dict of SHIFT_KEYS (displacement_summary): (0, 0) in a registered row says the
    output moved as the input did. On the device the row's one or two queries go through one musica_sim_displace call; on the host the
    restatement runs on the same planes; both summarise exact integer tables with one function, so the two agree to the last bit.
    displacement_tiles: each *_shift dict also carries "tile_tables" ((tiles_y, tiles_x, S, S) uint32) and "size" ((w, h) of its
    region), what displacement_maps draws. With displacement=0 the rows and the launches are exactly as before.

    scales: S > 0 (at most SIM_MAX_SCALES) says at which spatial scale the output changed (multiscale_similarities). Every comparison
    dict of a row gains a sibling: direct_scales, registered_scales and, with a vendor image, reference_scales and
    registered_reference_scales; present exactly where the original is and None exactly where it is None. Each is a dict of SCALES_KEYS:
    ms_ssim, scales and the lists ssim, cs, lum, mse of length `scales`, a comparison using min(S, max_scales of its region). On the
    device the row's queries go through one musica_sim_multiscale call per distinct scale count; on the host the restatement scores
    the same crops. With scales=0 the rows and the launches are exactly as before.

    ensemble: K > 0 (at most SIM_ENSEMBLE_MAX; needs runner.device_alterations, else ValueError) repeats every noise alteration K times and
    splits the change of the output into bias and noise (ensemble_statistics). Every row gains "ensemble": None for rows without noise,
    for c_sh_*, gn_* and pn_* a dict of "direct" (the full frame against the unaltered result, ENSEMBLE_KEYS), "registered" (the
    collimator's region; present exactly where the row's "registered" is, else None), "realisations" (K) and "per_realisation": "mean"
    and "std" (ddof = 1, 0 for K = 1) over the K realisations of the five SIM_METRICS of the direct comparison. The row's own keys and
    launches are untouched: the ensemble runs after the row is complete on a second context owned by the runner
    (runner.ensemble_context, batch runner.ensemble_batch) that holds the raw image as its source and the unaltered result in its slot 0.
    Realisation j of the row with ordinal o draws from the study's seed and the stream ensemble_stream(o, j); B realisations go through
    one step, musica_sim_ensemble_add and one musica_sim_compare call, and one musica_sim_ensemble_result call ends the row.
    ensemble_tiles: the "direct" dict also carries "tile_tables" ((tiles_y, tiles_x, 2) uint64) and "size", what ensemble_maps draws.
    With ensemble=0 nothing is created and the rows are exactly as before.

    covariance: a radius R > 0 (at most SIM_MAX_RADIUS; needs ensemble > 0, else ValueError) adds the texture of the noise: each noise
    row's "ensemble" dict gains "covariance": {"direct": ..., "registered": ...}, each a dict of COV_KEYS plus "nps_radial" and
    "hf_fraction" (covariance_row). The direct region is the full frame inset by R; the registered one the row's registered region inset
    by R, None where the row has none or an inset side is under 7. One musica_sim_ensemble_track call follows the row's reset and one
    musica_sim_ensemble_covariance call ends it. covariance_tiles: the dicts also carry "table" and "tile_tables". With covariance=0 the
    rows, keys and launches are exactly as before.

    blurs: radii of the resolution-loss rows (binomial_blur; BLURS for 1, 2, 4, 8), each in 1 .. BLUR_MAX_RADIUS, else ValueError before
    any work. None or empty adds nothing. Otherwise rows blur_<r> follow the d4_* rows: the raw image blurred with radius r (on the
    device: alter_blur), "direct" against the unaltered result (how much of the input's resolution loss reaches the output),
    "registered" over the frame inset by r (roi_blur) against the unaltered result blurred with the same radius (what a linear,
    shift-invariant processor would not show; None when the inset frame has a side under 8). On the device that reference goes into
    slot 1 and the blurred vendor image into slot 3 (musica_sim_blur_reference). Like the d4 rows they draw nothing from `rng` and take
    no ordinal; vendor, tone, scales and displacement apply to them as to a d4 row."""
    rng = rng or np.random.default_rng(0)
    n = raw.shape[0]
    if vendor is not None:
        vendor = np.asarray(vendor)
        want = (n - 2 * PROCESSING_MARGIN,) * 2
        if vendor.shape != want or vendor.dtype not in (np.uint8, np.uint16):
            raise ValueError("vendor image must be a %d x %d uint8 or uint16 array, got %r %s" % (want + (vendor.shape, vendor.dtype)))
    keys = ("alteration", "direct", "registered", "mean_cnr") + (() if vendor is None else ("reference", "registered_reference"))
    if tone:
        keys += tuple(TONE_KEYS[k] for k in keys if k in TONE_KEYS)
    displacement = int(displacement)
    if displacement and not 1 <= displacement <= mp.SIM_MAX_RADIUS:
        raise ValueError("displacement radius %d is not in 1 .. %d" % (displacement, mp.SIM_MAX_RADIUS))
    if displacement:
        keys += ("direct_shift", "registered_shift")
    scales = int(scales)
    if scales and not 1 <= scales <= mp.SIM_MAX_SCALES:
        raise ValueError("scales %d is not in 1 .. %d" % (scales, mp.SIM_MAX_SCALES))
    if scales:
        keys += tuple(SCALE_ROW_KEYS[k] for k in keys if k in SCALE_ROW_KEYS)
    ensemble = int(ensemble)
    if ensemble and not 1 <= ensemble <= mp.SIM_ENSEMBLE_MAX:
        raise ValueError("ensemble %d is not in 1 .. %d" % (ensemble, mp.SIM_ENSEMBLE_MAX))
    if ensemble and not getattr(runner, "device_alterations", False):
        raise ValueError("an ensemble repeats the device's noise alterations: it needs a runner with device_alterations")
    if ensemble:
        keys += ("ensemble",)
    covariance = int(covariance)
    if covariance and not 1 <= covariance <= mp.SIM_MAX_RADIUS:
        raise ValueError("covariance radius %d is not in 1 .. %d" % (covariance, mp.SIM_MAX_RADIUS))
    if covariance and not ensemble:
        raise ValueError("covariance is taken over the realisations of an ensemble: give ensemble > 0")
    shutters = scaled(SHUTTERS, n) if shutters is None else shutters
    translations = scaled(TRANSLATIONS, n) if translations is None else translations
    rotations = ROTATIONS if rotations is None else rotations
    sigmas = GAUSS_SIGMAS if sigmas is None else sigmas
    factors = POISSON_FACTORS if factors is None else factors
    symmetries = [int(e) for e in (symmetries or ())]
    for e in symmetries:
        if not 0 <= e <= 7:
            raise ValueError("symmetry element %d is not in 0 .. 7" % e)
    blurs = [int(r) for r in (blurs or ())]
    for r in blurs:
        if not 1 <= r <= mp.BLUR_MAX_RADIUS:
            raise ValueError("blur radius %d is not in 1 .. %d" % (r, mp.BLUR_MAX_RADIUS))
    device = getattr(runner, "device_metrics", False)
    alter_on_device = getattr(runner, "device_alterations", False)
    ref8 = vendor_to_u8(vendor) if vendor is not None and not device else None   # the host metrics' vendor image
    unalt = runner.run(raw)
    shape = unalt.shape
    full = (0, 0, 0, 0, shape[1], shape[0])

    def on_device(queries):
        return [{k: r[k] for k in mp.SIM_METRICS} for r in runner.proc.sim_compare(queries)]

    def tone_on_device(queries):
        """The JOINT_METRICS of a row's queries (at most four): one musica_sim_joint call, every query's slot remapped with its tone_lut
        into a slot of its own from SLOT_TONE on, then one musica_sim_compare call over the same regions for tone_ssim."""
        res = runner.proc.sim_joint(queries)
        for i, (q, r) in enumerate(zip(queries, res)):
            runner.proc.sim_remap_reference(SLOT_TONE + i, q[1], r["tone_lut"])
        scored = runner.proc.sim_compare([(q[0], SLOT_TONE + i) + tuple(q[2:]) for i, q in enumerate(queries)])
        for r, c in zip(res, scored):
            r["tone_ssim"] = c["ssim"]
        return [{k: r[k] for k in mp.JOINT_METRICS} for r in res]

    def scales_on_device(queries):
        """The SCALES_KEYS of a row's queries: one musica_sim_multiscale call per distinct scale count, results in the queries' order."""
        counts = [min(scales, max_scales(q[6], q[7])) for q in queries]
        out = [None] * len(queries)
        for n in sorted(set(counts)):
            idx = [i for i, c in enumerate(counts) if c == n]
            for i, r in zip(idx, runner.proc.sim_multiscale([queries[i] for i in idx], n)):
                out[i] = {k: r[k] for k in SCALES_KEYS}
        return out

    def scales_on_host(a, b):
        r = multiscale_similarities(a, b, min(scales, max_scales(a.shape[1], a.shape[0])))
        return {k: r[k] for k in SCALES_KEYS}

    def shift_summary(table, region, tiles, tiles_off, tile_tables):
        out = displacement_summary(table, region[4] * region[5], tiles, tiles_off)
        if displacement_tiles:
            out["tile_tables"], out["size"] = tile_tables, (region[4], region[5])
        return out

    def shifts_on_device(comparisons):
        """comparisons: (slot, region) pairs, region already inset (None: no comparison). One musica_sim_displace call for those present."""
        present = [(slot, region) for slot, region in comparisons if region is not None]
        res = iter(runner.proc.sim_displace([(0, slot) + region for slot, region in present], displacement, tables=True,
                                            tiles=displacement_tiles) if present else [])
        out = []
        for slot, region in comparisons:
            r = next(res) if region is not None else None
            out.append(None if r is None else shift_summary(r["table"], region, r["tiles_x"] * r["tiles_y"], r["tiles_off"], r.get("tile_tables")))
        return out

    def shift_on_host(a, b, region):
        """The same from the restatement: a the output, b the full plane it is compared with, region already inset (None: no comparison)."""
        if region is None:
            return None
        tt = displacement_tile_tables(a, b, region, displacement)
        return shift_summary(tt.astype(np.int64).sum(axis=(0, 1)), region, tt.shape[0] * tt.shape[1], displacement_tiles_off(tt), tt)

    first = {"alteration": "unaltered", "registered": None, "registered_tone": None, "registered_shift": None, "registered_scales": None,
             "ensemble": None}
    if device:
        runner.proc.sim_capture(SLOT_UNALTERED)
        queries = [(0, SLOT_UNALTERED) + full]
        if vendor is not None:
            runner.proc.sim_set_vendor_reference(SLOT_VENDOR, vendor)
            queries.append((0, SLOT_VENDOR) + full)
        res = on_device(queries)
        first["direct"] = res[0]
        if vendor is not None:
            first["reference"] = res[1]
        if tone:
            res = tone_on_device(queries)
            first["direct_tone"] = res[0]
            if vendor is not None:
                first["reference_tone"] = res[1]
        if displacement:
            first["direct_shift"] = shifts_on_device([(SLOT_UNALTERED, _inset(full, displacement))])[0]
        if scales:
            res = scales_on_device(queries)
            first["direct_scales"] = res[0]
            if vendor is not None:
                first["reference_scales"] = res[1]
    else:
        if displacement:
            first["direct_shift"] = shift_on_host(unalt, unalt, _inset(full, displacement))
        first["direct"] = similarities(unalt, unalt)
        if vendor is not None:
            first["reference"] = similarities(unalt, ref8)
        if tone:
            first["direct_tone"] = tone_similarities(unalt, unalt)
            if vendor is not None:
                first["reference_tone"] = tone_similarities(unalt, ref8)
        if scales:
            first["direct_scales"] = scales_on_host(unalt, unalt)
            if vendor is not None:
                first["reference_scales"] = scales_on_host(unalt, ref8)
    first["mean_cnr"] = runner.mean_cnr() if runner.proc else None
    rows = [{k: first[k] for k in keys if k in first}]

    if alter_on_device:
        runner.proc.alter_set_source(raw)
        seed = int(rng.integers(0, 2 ** 63))
    noisy = {}   # row name -> (ordinal, alter(proc, stream, image_index)): the noise rows, for their ensembles
    if ensemble:
        eproc = runner.ensemble_context(ensemble)
        eproc.alter_set_source(raw)
        for i in range(eproc.batch):     # every image of the batch holds a valid input, whatever the last chunk leaves unused
            eproc.alter_none(i)
        eproc.sim_set_reference(SLOT_UNALTERED, runner.proc.sim_get_reference(SLOT_UNALTERED))

    def ensemble_of(name, registered):
        """The "ensemble" value of a completed row: None unless it is a noise row. registered: the region of its registered comparison
        (None: the row has none)."""
        if name not in noisy:
            return None
        ordinal, alter = noisy[name]
        regions = [full] + ([registered] if registered is not None else [])
        per = {k: [] for k in mp.SIM_METRICS}
        eproc.sim_ensemble_reset()
        if covariance:
            tracked = [_inset(full, covariance), _inset(registered, covariance) if registered is not None else None]
            if tracked[0] is None:
                raise ValueError("covariance radius %d leaves no 7 x 7 region of the %d x %d output" % (covariance, full[4], full[5]))
            eproc.sim_ensemble_track([(0, SLOT_UNALTERED) + r for r in tracked if r is not None], covariance)
        for j0 in range(0, ensemble, eproc.batch):
            count = min(eproc.batch, ensemble - j0)
            for i in range(count):
                alter(eproc, ensemble_stream(ordinal, j0 + i), i)
            if not eproc.execute_device():
                raise RuntimeError("musica_execute_device failed: " + mp.last_error())
            eproc.sim_ensemble_add(0, count)
            for r in eproc.sim_compare([(i, SLOT_UNALTERED) + full for i in range(count)]):
                for k in mp.SIM_METRICS:
                    per[k].append(r[k])
        res = eproc.sim_ensemble_result([(0, SLOT_UNALTERED) + r for r in regions], tiles=ensemble_tiles)
        dicts = [ensemble_summary(*[r[k] for k in ("sq_bias_sum", "var_sum", "sq_err_sum", "bias_sum", "abs_bias_max", "var_max", "realisations")],
                                  g[4], g[5]) for r, g in zip(res, regions)]
        if ensemble_tiles:
            dicts[0]["tile_tables"], dicts[0]["size"] = res[0]["tile_tables"], (full[4], full[5])
        out = {"direct": dicts[0], "registered": dicts[1] if registered is not None else None, "realisations": ensemble,
               "per_realisation": {"mean": {k: float(np.mean(v)) for k, v in per.items()},
                                   "std": {k: float(np.std(v, ddof=1)) if ensemble > 1 else 0.0 for k, v in per.items()}}}
        if covariance:
            cov = iter(eproc.sim_ensemble_covariance(tables=True, tiles=covariance_tiles))
            groups = []
            for r in tracked:
                if r is None:
                    groups.append(None)
                    continue
                c = next(cov)
                d = covariance_row(c["table"], c["realisations"], r[4], r[5])
                if covariance_tiles:
                    d["table"], d["tile_tables"] = c["table"], c["tile_tables"]
                groups.append(d)
            out["covariance"] = {"direct": groups[0], "registered": groups[1]}
        return out

    def add(name, host, dev, reg=None, region=None, slot=None, plane=None):
        """One row of study() below, scored the way the runner's mode asks for."""
        row = {"alteration": name, "registered": None, "registered_reference": None, "registered_tone": None, "registered_reference_tone": None,
               "registered_shift": None, "registered_scales": None, "registered_reference_scales": None}
        if alter_on_device:
            dev()
            runner.run_resident()
        elif device:
            runner.run_device(host())
        if device:
            queries = [(0, SLOT_UNALTERED) + full]
            if vendor is not None:
                queries.append((0, SLOT_VENDOR) + full)
            registered = None   # (slot, region) of the registered comparison
            if region is not None:
                sl, r = slot(), region()
                if r is not None and min(r[4], r[5]) >= 8:
                    registered = (sl, r)
                    queries.append((0, sl) + r)
                    if vendor is not None:
                        queries.append((0, VENDOR_SLOT[sl]) + r)
            for suffix, score in (("", on_device),) + ((("_tone", tone_on_device),) if tone else ()) + ((("_scales", scales_on_device),) if scales else ()):
                res = score(queries)
                row["direct" + suffix] = res.pop(0)
                if vendor is not None:
                    row["reference" + suffix] = res.pop(0)
                if res:
                    row["registered" + suffix] = res.pop(0)
                    if vendor is not None:
                        row["registered_reference" + suffix] = res.pop(0)
            if displacement:
                row["direct_shift"], row["registered_shift"] = shifts_on_device(
                    [(SLOT_UNALTERED, _inset(full, displacement)),
                     (registered[0], _inset(registered[1], displacement)) if registered else (None, None)])
        else:
            alt = runner.run(host())
            crop = reg(alt, unalt) if reg is not None else None
            if crop is not None and not (crop[0].size and crop[0].shape == crop[1].shape and min(crop[0].shape) >= 8):
                crop = None
            vcrop = reg(alt, ref8) if crop is not None and vendor is not None else None   # the same rectangles: ref8 has unalt's shape
            for suffix, score in (("", similarities),) + ((("_tone", tone_similarities),) if tone else ()) + ((("_scales", scales_on_host),) if scales else ()):
                row["direct" + suffix] = score(alt, unalt)
                if vendor is not None:
                    row["reference" + suffix] = score(alt, ref8)
                if crop is not None:
                    row["registered" + suffix] = score(*crop)
                    if vendor is not None:
                        row["registered_reference" + suffix] = score(*vcrop)
            if displacement:
                row["direct_shift"] = shift_on_host(alt, unalt, _inset(full, displacement))
                if crop is not None:
                    row["registered_shift"] = shift_on_host(alt, plane(), _inset(region(), displacement))
        row["mean_cnr"] = runner.mean_cnr() if runner.proc else None
        if ensemble:   # device path (an ensemble needs device alterations): `registered` is the row's own (slot, region)
            row["ensemble"] = ensemble_of(name, registered[1] if registered else None)
        rows.append({k: row[k] for k in keys})

    def moved_slot(d, move_reference, moved_unalt):
        """The unaltered result (and the vendor image) moved as the row moves its input, into SLOT_ROTATED (SLOT_VENDOR_ROTATED)."""
        if alter_on_device:
            move_reference(SLOT_ROTATED, SLOT_UNALTERED, d)
        else:
            runner.proc.sim_set_reference(SLOT_ROTATED, moved_unalt(unalt, d))
        if vendor is not None:
            move_reference(SLOT_VENDOR_ROTATED, SLOT_VENDOR, d)
        return SLOT_ROTATED

    def study():
        """Every alteration of the study once, in the rows' order, as add()'s arguments: name; host() the altered raw image; dev() the
        call that writes it into the resident input buffer; reg(alt, unalt) the host's registration crop; region() the region of the
        same comparison (None: no registration); slot() the reference slot its b side lies in on the device, filled by that call where
        it is not the unaltered result's; plane() the full host plane it lies in. The noise rows have only the first three. add() makes a
        row's calls before the next row is built: the rows' order is the order of the `rng` draws. The device's noise draws take the
        row's ordinal in the study as their stream; the d4 and blur rows draw nothing and take no ordinal."""
        p, ordinal = runner.proc, itertools.count(1)
        for s in shutters:
            k = next(ordinal)
            noisy["c_sh_%d" % s] = (k, lambda q, stream, i: q.alter_collimator(s, s, seed, stream, i))
            yield ("c_sh_%d" % s, lambda: apply_collimator(raw, s, s, rng), lambda k=k: p.alter_collimator(s, s, seed, k),
                   lambda a, u: register_collimator(a, u, s), lambda: roi_collimator(shape, s), lambda: SLOT_UNALTERED, lambda: unalt)
        for name, tx, ty, register, roi in (("t_x_%d", 1, 0, register_translation_x, roi_translation_x), ("t_y_%d", 0, 1, register_translation_y, roi_translation_y)):
            for t in translations:
                next(ordinal)   # every row before the d4 rows takes one, drawing or not
                yield (name % t, lambda: clamp_translation(raw, tx * t, ty * t), lambda: p.alter_translate(tx * t, ty * t),
                       lambda a, u: register(a, u, t), lambda: roi(shape, t), lambda: SLOT_UNALTERED, lambda: unalt)
        for d in rotations:
            next(ordinal)
            yield ("r_%d" % d, lambda: clamp_rotate(raw, d), lambda: p.alter_rotate(d), lambda a, u: register_rotation(a, u, d),
                   lambda: roi_rotation(shape, d), lambda: moved_slot(d, p.sim_rotate_reference, rotated_reference), lambda: rotated_reference(unalt, d))
        for sg in sigmas:
            k = next(ordinal)
            noisy["gn_%s" % sg] = (k, lambda q, stream, i: q.alter_gaussian(0.0, sg, seed, stream, i))
            yield ("gn_%s" % sg, lambda: add_gaussian_noise(raw, 0.0, sg, rng), lambda k=k: p.alter_gaussian(0.0, sg, seed, k))
        for f in factors:
            k = next(ordinal)
            noisy["pn_%s" % f] = (k, lambda q, stream, i: q.alter_poisson(f, seed, stream, i))
            yield ("pn_%s" % f, lambda: apply_quantum_noise(raw, f, rng), lambda k=k: p.alter_poisson(f, seed, k))
        for e in symmetries:
            yield ("d4_%d" % e, lambda: apply_symmetry(raw, e), lambda: p.alter_symmetry(e), lambda a, u: register_symmetry(a, u, e),
                   lambda: roi_symmetry(shape), lambda: moved_slot(e, p.sim_transform_reference, apply_symmetry), lambda: apply_symmetry(unalt, e))
        for r in blurs:
            yield ("blur_%d" % r, lambda: binomial_blur(raw, r), lambda: p.alter_blur(r), lambda a, u: register_blur(a, u, r),
                   lambda: roi_blur(shape, r), lambda: moved_slot(r, p.sim_blur_reference, binomial_blur), lambda: binomial_blur(unalt, r))

    for row in study():
        add(*row)
    return rows


# ---- command line: the reference's three CSV files (script.py:223-330) -------------------------
CSV_HEADER = ['raw file', 'alteration', 'altered vs unaltered mse', 'altered vs unaltered ssim', 'altered vs unaltered histogram distance',
              'altered vs reference mse', 'altered vs reference ssim', 'altered vs reference histogram distance',
              'normalized altered vs reference mse', 'normalized altered vs reference ssim',
              'normalized altered vs reference histogram distance']


REF_CSV_HEADER = ['raw file', 'mse similarity', 'ssim similarity', 'histogram distance']   # ref_similarities.csv (script.py:285-290)
TONE_CSV_NAMES = ('mutual information', 'normalized mutual information', 'correlation ratio', 'tone-matched mse', 'tone-matched ssim')   # JOINT_METRICS' order
TONE_CSV_GROUPS = (('direct_tone', 'altered vs unaltered'), ('registered_tone', 'registered vs unaltered'),
                   ('reference_tone', 'altered vs reference'), ('registered_reference_tone', 'registered vs reference'))


SHIFT_CSV_NAMES = ('dx', 'dy', 'sub dx', 'sub dy', 'mse at zero', 'mse at best', 'tiles', 'tiles off')   # SHIFT_KEYS' order
SHIFT_CSV_GROUPS = (('direct_shift', 'direct'), ('registered_shift', 'registered'))
SHIFT_CSV_HEADER = ['raw file', 'alteration'] + ['%s %s' % (g, m) for _, g in SHIFT_CSV_GROUPS for m in SHIFT_CSV_NAMES]   # displacement.csv


SCALE_CSV_GROUPS = tuple((SCALE_ROW_KEYS[k], g) for k, g in (("direct", "altered vs unaltered"), ("registered", "registered vs unaltered"),
                                                               ("reference", "altered vs reference"), ("registered_reference", "registered vs reference")))
SCALE_CSV_METRICS = ("ssim", "cs", "mse")   # per scale 0 .. 4, behind ms_ssim and scales


ENSEMBLE_CSV_NAMES = (("mean_shift", "mean shift"), ("bias_rms", "bias rms"), ("noise_rms", "noise rms"), ("bias_fraction", "bias fraction"), ("mse", "mse"))
ENSEMBLE_CSV_METRICS = ("mse", "ssim", "histogram intersection", "histogram distance", "histogram bhattacharyya")   # SIM_METRICS' order
ENSEMBLE_CSV_HEADER = ['raw file', 'alteration', 'realisations'] + ['%s %s' % (g, m) for g in ("direct", "registered") for _, m in ENSEMBLE_CSV_NAMES] + \
                      ['per-realisation %s %s' % (m, w) for m in ENSEMBLE_CSV_METRICS for w in ("mean", "std")]   # ensemble.csv


COV_CSV_NAMES = (("noise_var", "noise var"), ("rho_x", "rho x"), ("rho_y", "rho y"), ("corr_area", "correlation area"), ("hf_fraction", "hf fraction"))


def covariance_csv_header(radius):
    """noise_covariance.csv of a study with covariance=radius: the groups' numbers, then the radial spectrum of the direct group."""
    return ['raw file', 'alteration', 'realisations', 'radius'] + ['%s %s' % (g, m) for g in ("direct", "registered") for _, m in COV_CSV_NAMES] + \
           ['direct nps radius %d' % i for i in range(int(radius) + 1)]


def scale_csv_header(with_reference):
    """scale_robustness.csv's columns: per group ms_ssim, scales, then ssim, cs and mse of scales 0 .. 4; the two vendor groups only for
    studies that have a vendor image."""
    return ['raw file', 'alteration'] + [c for _, g in SCALE_CSV_GROUPS[:4 if with_reference else 2] for c in
                                         ['%s ms-ssim' % g, '%s scales' % g] +
                                         ['%s %s scale %d' % (g, m, s) for m in SCALE_CSV_METRICS for s in range(mp.SIM_MAX_SCALES)]]


def _scale_csv_cells(t):
    if t is None:
        return [""] * (2 + len(SCALE_CSV_METRICS) * mp.SIM_MAX_SCALES)
    return [t["ms_ssim"], t["scales"]] + [t[m][s] if s < t["scales"] else "" for m in SCALE_CSV_METRICS for s in range(mp.SIM_MAX_SCALES)]


def tone_csv_header(with_reference):
    """tone_robustness.csv's columns: the five JOINT_METRICS per group, the two vendor groups only for studies that have a vendor image."""
    return ['raw file', 'alteration'] + ['%s %s' % (g, m) for _, g in TONE_CSV_GROUPS[:4 if with_reference else 2] for m in TONE_CSV_NAMES]


def normalized_vs_reference(ref, ovd):
    """m_sim_alt's three normalised values (script.py:272-274): ref_mse / ovd_mse, ref_ssim / ovd_ssim and
    (ref_hist - ovd_hist) / (1 - ovd_hist), with ovd the unaltered result vs the vendor image. IEEE f64 division: a zero denominator
    gives inf or nan (the reference would raise ZeroDivisionError and stop the study)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return [float(np.float64(ref["mse"]) / np.float64(ovd["mse"])), float(np.float64(ref["ssim"]) / np.float64(ovd["ssim"])),
                float((np.float64(ref["hist_distance"]) - ovd["hist_distance"]) / (1.0 - np.float64(ovd["hist_distance"])))]


def write_studies_csvs(studies, out_dir, mean_cnr=True):
    """The reference's output files for several raw images: `studies` is a list of (raw_name, rows) pairs (run_study's rows), written
    in order into one direct_robustness.csv / reg_based_robustness.csv with the reference's column layout (script.py:223-330), plus
    mean_cnr.csv (what test/mean_cnr/script.py reports per alteration).

    The six "vs reference" columns compare with the vendor-processed image. For a study run with one (rows[0] has "reference"): the
    altered result vs that image (reg_based_robustness.csv: the registered crops), then normalized_vs_reference against the study's
    full-image unaltered-vs-vendor values, as m_sim_alt and m_sim_norm_alt do; ref_similarities.csv gets one row of those values per
    such study and is written only when there is one. Studies without a vendor image leave the six columns empty.

    Studies run with tone=True (rows[0] has "direct_tone") also get tone_robustness.csv: one line per row, the unaltered one included
    (with a vendor image it carries the unaltered-vs-vendor numbers), the five JOINT_METRICS of the direct and of the registered
    comparison, then, when any study has a vendor image, of the two comparisons with it. Cells without a comparison are empty. The
    other files are written as without it.

    Studies run with a displacement radius (rows[0] has "direct_shift") also get displacement.csv: one line per row, the unaltered one
    included, the SHIFT_KEYS of the direct and of the registered comparison; cells without a comparison are empty.

    Studies run with scales (rows[0] has "direct_scales") also get scale_robustness.csv (scale_csv_header): one line per row, the
    unaltered one included; cells without a comparison, and of scales beyond a comparison's count, are empty.

    Studies run with ensemble=K (rows[0] has "ensemble") also get ensemble.csv (ENSEMBLE_CSV_HEADER): one line per noise row, K, the
    mean shift, bias rms, noise rms, bias fraction and mse of the direct and of the registered ensemble (empty without one), then the mean
    and standard deviation over the realisations of the five similarity metrics.

    Studies run with covariance=R (their noise rows' "ensemble" has "covariance") also get noise_covariance.csv
    (covariance_csv_header): one line per noise row, K, R, the noise variance, rho x, rho y, correlation area and high-frequency
    fraction of the direct and of the registered region (empty without one), then the radial noise power spectrum of the direct one."""
    os.makedirs(out_dir, exist_ok=True)
    ovds = []

    def ref_columns(ref, ovd):
        if ovd is None:
            return [""] * 6
        return [ref["mse"], ref["ssim"], ref["hist_distance"]] + normalized_vs_reference(ref, ovd)

    with open(os.path.join(out_dir, "direct_robustness.csv"), "w", newline="") as fd, \
            open(os.path.join(out_dir, "reg_based_robustness.csv"), "w", newline="") as fr:
        wd, wr = csv.writer(fd), csv.writer(fr)
        wd.writerow(CSV_HEADER)
        wr.writerow(CSV_HEADER)
        for raw_name, rows in studies:
            ovd = next((r.get("reference") for r in rows if r["alteration"] == "unaltered"), None)
            if ovd is not None:
                ovds.append([raw_name, ovd["mse"], ovd["ssim"], ovd["hist_distance"]])
            for r in rows:
                if r["alteration"] == "unaltered":
                    continue
                d = r["direct"]
                wd.writerow([raw_name, r["alteration"], d["mse"], d["ssim"], d["hist_distance"]] + ref_columns(r.get("reference"), ovd))
                if r["registered"] is not None:
                    g = r["registered"]
                    wr.writerow([raw_name, r["alteration"], g["mse"], g["ssim"], g["hist_distance"]] +
                                ref_columns(r.get("registered_reference"), ovd))
    if mean_cnr:
        with open(os.path.join(out_dir, "mean_cnr.csv"), "w", newline="") as fc:
            wc = csv.writer(fc)
            wc.writerow(["raw file", "alteration", "mean cnr"])
            for raw_name, rows in studies:
                for r in rows:
                    wc.writerow([raw_name, r["alteration"], r["mean_cnr"]])
    if ovds:
        with open(os.path.join(out_dir, "ref_similarities.csv"), "w", newline="") as fs:
            ws = csv.writer(fs)
            ws.writerow(REF_CSV_HEADER)
            ws.writerows(ovds)
    toned = [(raw_name, rows) for raw_name, rows in studies if rows and "direct_tone" in rows[0]]
    if toned:
        groups = TONE_CSV_GROUPS[:4 if any("reference_tone" in rows[0] for _, rows in toned) else 2]
        with open(os.path.join(out_dir, "tone_robustness.csv"), "w", newline="") as ft:
            wt = csv.writer(ft)
            wt.writerow(tone_csv_header(len(groups) == 4))
            for raw_name, rows in toned:
                for r in rows:
                    cells = []
                    for key, _ in groups:
                        t = r.get(key)
                        cells += [""] * len(mp.JOINT_METRICS) if t is None else [t[k] for k in mp.JOINT_METRICS]
                    wt.writerow([raw_name, r["alteration"]] + cells)
    shifted = [(raw_name, rows) for raw_name, rows in studies if rows and "direct_shift" in rows[0]]
    if shifted:
        with open(os.path.join(out_dir, "displacement.csv"), "w", newline="") as fs:
            ws = csv.writer(fs)
            ws.writerow(SHIFT_CSV_HEADER)
            for raw_name, rows in shifted:
                for r in rows:
                    cells = []
                    for key, _ in SHIFT_CSV_GROUPS:
                        t = r.get(key)
                        cells += [""] * len(SHIFT_KEYS) if t is None else [t[k] for k in SHIFT_KEYS]
                    ws.writerow([raw_name, r["alteration"]] + cells)


    scored = [(raw_name, rows) for raw_name, rows in studies if rows and "direct_scales" in rows[0]]
    if scored:
        groups = SCALE_CSV_GROUPS[:4 if any("reference_scales" in rows[0] for _, rows in scored) else 2]
        with open(os.path.join(out_dir, "scale_robustness.csv"), "w", newline="") as fs:
            ws = csv.writer(fs)
            ws.writerow(scale_csv_header(len(groups) == 4))
            for raw_name, rows in scored:
                for r in rows:
                    ws.writerow([raw_name, r["alteration"]] + [c for key, _ in groups for c in _scale_csv_cells(r.get(key))])
    ensembles = [(raw_name, rows) for raw_name, rows in studies if rows and "ensemble" in rows[0]]
    if ensembles:
        with open(os.path.join(out_dir, "ensemble.csv"), "w", newline="") as fe:
            we = csv.writer(fe)
            we.writerow(ENSEMBLE_CSV_HEADER)
            for raw_name, rows in ensembles:
                for r in rows:
                    e = r["ensemble"]
                    if e is None:
                        continue
                    cells = []
                    for key in ("direct", "registered"):
                        cells += [""] * len(ENSEMBLE_CSV_NAMES) if e[key] is None else [e[key][k] for k, _ in ENSEMBLE_CSV_NAMES]
                    per = e["per_realisation"]
                    we.writerow([raw_name, r["alteration"], e["realisations"]] + cells + [per[w][k] for k in mp.SIM_METRICS for w in ("mean", "std")])
    covs = [(raw_name, [r for r in rows if r.get("ensemble") and "covariance" in r["ensemble"]]) for raw_name, rows in ensembles]
    covs = [(raw_name, rows) for raw_name, rows in covs if rows]
    if covs:
        radius = covs[0][1][0]["ensemble"]["covariance"]["direct"]["radius"]
        with open(os.path.join(out_dir, "noise_covariance.csv"), "w", newline="") as fc:
            wc = csv.writer(fc)
            wc.writerow(covariance_csv_header(radius))
            for raw_name, rows in covs:
                for r in rows:
                    e = r["ensemble"]
                    cells = []
                    for key in ("direct", "registered"):
                        g = e["covariance"][key]
                        cells += [""] * len(COV_CSV_NAMES) if g is None else [g[k] for k, _ in COV_CSV_NAMES]
                    wc.writerow([raw_name, r["alteration"], e["realisations"], radius] + cells + list(e["covariance"]["direct"]["nps_radial"]))


def write_ensemble_maps(studies, out_dir):
    """Two 8-bit BMPs per noise row of studies run with ensemble_tiles (ensemble_maps: one pixel per 64 x 64 tile of the full frame):
    <raw>_<alteration>_bias.bmp, the tile's bias rms against the unaltered result, and <raw>_<alteration>_noise.bmp, its noise rms, in
    gray levels. Returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for raw_name, rows in studies:
        stem = os.path.splitext(os.path.basename(raw_name.replace("\\", "/")))[0]
        for r in rows:
            e = r.get("ensemble")
            if e is None or "tile_tables" not in e["direct"]:
                continue
            for what, img in zip(("bias", "noise"), ensemble_maps(e["direct"]["tile_tables"], *e["direct"]["size"], e["realisations"])):
                path = os.path.join(out_dir, "%s_%s_%s.bmp" % (stem, r["alteration"], what))
                if not mp.write_bmp_gray(path, img):
                    raise RuntimeError("writing %s failed: %s" % (path, mp.last_error()))
                written.append(path)
    return written


def write_covariance_maps(studies, out_dir):
    """One 8-bit BMP per noise row of studies run with covariance_tiles: <raw>_<alteration>_nps.bmp, the centred noise power spectrum of
    the direct region (nps_map: S x S pixels, the zero frequency in the middle, log-scaled). Returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for raw_name, rows in studies:
        stem = os.path.splitext(os.path.basename(raw_name.replace("\\", "/")))[0]
        for r in rows:
            e = r.get("ensemble")
            g = e["covariance"]["direct"] if e and "covariance" in e else None
            if g is None or "table" not in g:
                continue
            path = os.path.join(out_dir, "%s_%s_nps.bmp" % (stem, r["alteration"]))
            if not mp.write_bmp_gray(path, nps_map(g["table"], g["realisations"], g["pixels"])):
                raise RuntimeError("writing %s failed: %s" % (path, mp.last_error()))
            written.append(path)
    return written


def write_displacement_maps(studies, out_dir):
    """Two 8-bit BMPs per registered row of studies run with displacement_tiles (displacement_maps: one pixel per 64 x 64 tile):
    <raw>_<alteration>_rmse.bmp, the tile RMSE at the zero shift, and <raw>_<alteration>_shift.bmp, the length of the tile's best shift.
    Returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for raw_name, rows in studies:
        stem = os.path.splitext(os.path.basename(raw_name.replace("\\", "/")))[0]
        for r in rows:
            t = r.get("registered_shift")
            if t is None or "tile_tables" not in t:
                continue
            for what, img in zip(("rmse", "shift"), displacement_maps(t["tile_tables"], *t["size"])):
                path = os.path.join(out_dir, "%s_%s_%s.bmp" % (stem, r["alteration"], what))
                if not mp.write_bmp_gray(path, img):
                    raise RuntimeError("writing %s failed: %s" % (path, mp.last_error()))
                written.append(path)
    return written


def write_study_csvs(rows, out_dir, raw_name, mean_cnr=True):
    """write_studies_csvs for one raw image: direct_robustness.csv / reg_based_robustness.csv with the reference's column layout,
    mean_cnr.csv, and (rows of a study with a vendor image) the "vs reference" columns and ref_similarities.csv."""
    write_studies_csvs([(raw_name, rows)], out_dir, mean_cnr=mean_cnr)


def read_manifest(path):
    """The images of a --manifest file: one `raw[,reference]` per line, `#` starts a comment, blank lines are skipped. Paths are
    relative to the manifest's directory (either slash separates directories, so the reference's `foot\\image.raw` works as written).
    Returns [(raw as written, raw path, reference path or None)]."""
    base = os.path.dirname(os.path.abspath(path))

    def resolve(p):
        return os.path.join(base, *[s for s in p.replace("\\", "/").split("/") if s]) if not os.path.isabs(p) else p

    entries = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            parts = [s.strip() for s in line.split(",")]
            if len(parts) > 2 or not all(parts):
                raise ValueError("%s:%d: expected `raw[,reference]`, got %r" % (path, ln, line))
            entries.append((parts[0], resolve(parts[0]), resolve(parts[1]) if len(parts) == 2 else None))
    if not entries:
        raise ValueError("%s: no images" % path)
    return entries


def run_studies(entries, runner, **study_args):
    """run_study over several raw images through one runner: `entries` as read_manifest returns them (raw paths of the runner's size;
    a reference: the vendor DICOM, read with dicom.read_dicom_gray). Every image gets a fresh np.random.default_rng(0), so its rows are
    those of a study of that image alone. Returns [(raw as written, rows)], for write_studies_csvs."""
    from .dicom import read_dicom_gray
    from .processing import read_raw
    studies = []
    for name, raw_path, ref_path in entries:
        raw = read_raw(raw_path, runner.n)
        if raw is None:
            raise ValueError("%s: not a raw file of %d x %d pixels (256-byte header + N*N uint16)" % (raw_path, runner.n, runner.n))
        vendor = read_dicom_gray(ref_path) if ref_path else None
        studies.append((name, run_study(raw, runner, rng=np.random.default_rng(0), vendor=vendor, **study_args)))
    return studies


def symmetry_list(text):
    """--symmetries' comma list of elements 0 .. 7."""
    import argparse
    try:
        elements = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected a comma-separated list of elements 0 .. 7, got %r" % text)
    if not elements or any(not 0 <= e <= 7 for e in elements):
        raise argparse.ArgumentTypeError("symmetry elements are 0 .. 7, got %r" % text)
    return elements


def blur_list(text):
    """--blurs' comma list of radii 1 .. BLUR_MAX_RADIUS."""
    import argparse
    try:
        radii = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected a comma-separated list of radii 1 .. %d, got %r" % (mp.BLUR_MAX_RADIUS, text))
    if not radii or any(not 1 <= r <= mp.BLUR_MAX_RADIUS for r in radii):
        raise argparse.ArgumentTypeError("blur radii are 1 .. %d, got %r" % (mp.BLUR_MAX_RADIUS, text))
    return radii


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Metamorphic study of raw images (or a seeded phantom) on the HIP MUSICA path")
    ap.add_argument("--raw", help="raw file: 256-byte header + N*N little-endian uint16 (test/standalone/main.cpp:54-75)")
    ap.add_argument("--reference", help="the vendor-processed DICOM of --raw (or of the phantom): fills the \"vs reference\" columns and "
                                        "writes ref_similarities.csv (script.py:370-411)")
    ap.add_argument("--manifest", help="text file with one `raw[,reference]` per line (paths relative to it, # comments): every image "
                                       "through one runner into the same CSV files; excludes --raw and --reference")
    ap.add_argument("--phantom-seed", type=int, default=1, help="seed of the synthetic phantom used when --raw is absent")
    ap.add_argument("--size", type=int, default=3072, help="image side N (the reference's CLI fixes 3072)")
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--out", default="out", help="directory of the CSV files")
    ap.add_argument("--cli", action="store_true", help="run every image through the musica-standalone process (run_process, script.py:200-214)")
    ap.add_argument("--device-metrics", action="store_true", help="compute MSE, SSIM and the histogram distances on the GPU (musica_sim_compare)")
    ap.add_argument("--device-alterations", action="store_true",
                    help="generate the alterations on the GPU (musica_alter; implies --device-metrics); the noise rows then come from a "
                         "different, reproducible, random stream than the host study's")
    ap.add_argument("--symmetries", nargs="?", const=SYMMETRIES, default=None, type=symmetry_list, metavar="E,E,...",
                    help="add the rows d4_<e>: the raw image under elements of the square's symmetry group (1, 3: quarter turns, 2: half turn, "
                         "4: transpose, 5, 7: flips, 6: anti-transpose), compared over the whole frame; without a list, all seven")
    ap.add_argument("--blurs", nargs="?", const=BLURS, default=None, type=blur_list, metavar="R,R,...",
                    help="add the rows blur_<r>: the raw image under the exact binomial blur of radius r (1 .. 8; sigma = sqrt(r / 2) pixels), "
                         "compared directly and, inset by r, with the unaltered result blurred alike; without a list, 1,2,4,8")
    ap.add_argument("--tone", action="store_true",
                    help="add the joint-histogram tone metrics of every comparison (mutual information, correlation ratio, tone-matched mse and "
                         "ssim) and write them to tone_robustness.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_joint)")
    ap.add_argument("--displacement", type=int, default=0, metavar="R",
                    help="measure where the output went: exact block matching over all integer shifts within R (1 .. 16) pixels, per row the "
                         "direct and the registered comparison, written to displacement.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_displace)")
    ap.add_argument("--displacement-maps", metavar="DIR",
                    help="with --displacement: two 8-bit BMPs per registered row into DIR, one pixel per 64 x 64 tile: the tile RMSE at the zero "
                         "shift and the length of the tile's best shift")
    ap.add_argument("--scales", type=int, default=0, metavar="S",
                    help="say at which spatial scale the output changed: SSIM, its contrast-structure factor and mse at S (1 .. 5) scales of "
                         "2 x 2 pooling and their MS-SSIM product, per comparison, written to scale_robustness.csv; on the GPU with "
                         "--device-metrics / --device-alterations (musica_sim_multiscale)")
    ap.add_argument("--ensemble", type=int, default=0, metavar="K",
                    help="with --device-alterations: repeat every noise alteration K (1 .. 1024) times and split the change of the output into "
                         "bias against the unaltered result and noise, per pixel, written to ensemble.csv (musica_sim_ensemble_*)")
    ap.add_argument("--ensemble-batch", type=int, default=8, metavar="B", help="with --ensemble: realisations per step of the ensemble context")
    ap.add_argument("--ensemble-maps", metavar="DIR",
                    help="with --ensemble: two 8-bit BMPs per noise row into DIR, one pixel per 64 x 64 tile: the tile's bias rms and its noise rms")
    ap.add_argument("--covariance", type=int, default=0, metavar="R",
                    help="with --ensemble: the spatial auto-covariance of the output noise over the lags within R (1 .. 16) pixels, its "
                         "neighbour correlations, correlation area and noise power spectrum, written to noise_covariance.csv "
                         "(musica_sim_ensemble_track, musica_sim_ensemble_covariance)")
    ap.add_argument("--covariance-maps", metavar="DIR",
                    help="with --covariance: one 8-bit BMP per noise row into DIR: the centred noise power spectrum, log-scaled")
    args = ap.parse_args(argv)
    if args.covariance and not 1 <= args.covariance <= mp.SIM_MAX_RADIUS:
        ap.error("--covariance takes a radius of 1 .. %d pixels" % mp.SIM_MAX_RADIUS)
    if args.covariance and not args.ensemble:
        ap.error("--covariance is taken over the realisations of an ensemble: give --ensemble")
    if args.covariance_maps and not args.covariance:
        ap.error("--covariance-maps draws what --covariance measures: give a radius")
    if args.ensemble and not 1 <= args.ensemble <= mp.SIM_ENSEMBLE_MAX:
        ap.error("--ensemble takes a count of 1 .. %d realisations" % mp.SIM_ENSEMBLE_MAX)
    if args.ensemble and not args.device_alterations:
        ap.error("--ensemble repeats the device's noise alterations: give --device-alterations")
    if args.ensemble_maps and not args.ensemble:
        ap.error("--ensemble-maps draws what --ensemble measures: give a count")
    if args.ensemble_batch < 1:
        ap.error("--ensemble-batch takes at least 1")
    if args.scales and not 1 <= args.scales <= mp.SIM_MAX_SCALES:
        ap.error("--scales takes a count of 1 .. %d" % mp.SIM_MAX_SCALES)
    if args.displacement and not 1 <= args.displacement <= mp.SIM_MAX_RADIUS:
        ap.error("--displacement takes a radius of 1 .. %d pixels" % mp.SIM_MAX_RADIUS)
    if args.displacement_maps and not args.displacement:
        ap.error("--displacement-maps draws what --displacement measures: give a radius")
    if args.cli and args.device_alterations:
        ap.error("--device-alterations writes the in-process library's input buffer: it cannot be combined with --cli")
    if args.cli and args.device_metrics:
        ap.error("--device-metrics scores the in-process library's device output: it cannot be combined with --cli")
    if args.manifest and (args.raw or args.reference):
        ap.error("--manifest names every raw image and its reference: it cannot be combined with --raw or --reference")
    if args.manifest:
        entries = read_manifest(args.manifest)
    elif args.raw:
        from .processing import read_raw
        raw = read_raw(args.raw, args.size)
        name = os.path.basename(args.raw)
    else:
        from .phantom import phantom
        raw = phantom(args.size, args.phantom_seed, noise=4.0)
        name = "phantom_%d_seed%d" % (args.size, args.phantom_seed)
    if args.reference:
        from .dicom import read_dicom_gray
        vendor = read_dicom_gray(args.reference)
    runner = Runner(args.size, args.levels, use_cli=args.cli, device_metrics=args.device_metrics, device_alterations=args.device_alterations,
                    **({"ensemble_batch": args.ensemble_batch} if args.ensemble else {}))
    shift_args = {"displacement": args.displacement, "displacement_tiles": True} if args.displacement_maps else \
                 {"displacement": args.displacement} if args.displacement else {}
    if args.scales:
        shift_args["scales"] = args.scales
    if args.ensemble:
        shift_args.update(ensemble=args.ensemble, ensemble_tiles=bool(args.ensemble_maps))
    if args.covariance:
        shift_args.update(covariance=args.covariance, covariance_tiles=bool(args.covariance_maps))
    if args.blurs:
        shift_args["blurs"] = args.blurs
    try:
        if args.manifest:
            studies = run_studies(entries, runner, symmetries=args.symmetries, tone=args.tone, **shift_args)
        else:
            studies = [(name, run_study(raw, runner, rng=np.random.default_rng(0), vendor=vendor if args.reference else None,
                                        symmetries=args.symmetries, tone=args.tone, **shift_args))]
    finally:
        runner.close()
    write_studies_csvs(studies, args.out, mean_cnr=not args.cli)
    if args.displacement_maps:
        write_displacement_maps(studies, args.displacement_maps)
    if args.ensemble_maps:
        write_ensemble_maps(studies, args.ensemble_maps)
    if args.covariance_maps:
        write_covariance_maps(studies, args.covariance_maps)
    print("wrote %d alterations to %s" % (sum(len(rows) - 1 for _, rows in studies), args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

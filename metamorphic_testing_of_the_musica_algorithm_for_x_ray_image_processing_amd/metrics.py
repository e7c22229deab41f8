"""The host restatements of the study's metrics: numpy statements of what the musica_sim_* kernels compute (include/musica.h), which the
host study scores with and the GPU tests compare the kernels against. harness re-exports every name."""
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

from . import processing as mp


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


def warp_shifts(field, xs, ys):
    """harness.warp's interpolated displacements (s_0, s_1), two (len(ys), len(xs)) int64 arrays in 1 / 256 pixel, at the GRID coordinates
    xs (columns) and ys (rows), origin included: with cx = X >> 6, fx = X & 63 and likewise in y, per component
    s = ((64 - fy) ((64 - fx) d[cy, cx] + fx d[cy, cx + 1]) + fy ((64 - fx) d[cy + 1, cx] + fx d[cy + 1, cx + 1]) + 2048) >> 12.
    The field must hold the nodes cy + 1, cx + 1 of every coordinate (processing.warp_field checks a plane's)."""
    f = np.asarray(field).astype(np.int64)
    xs, ys = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64)
    cx, fx, cy, fy = xs >> 6, (xs & 63)[None, :], ys >> 6, (ys & 63)[:, None]
    out = []
    for c in (0, 1):
        d = f[:, :, c]
        top = (64 - fx) * d[cy][:, cx] + fx * d[cy][:, cx + 1]
        bottom = (64 - fx) * d[cy + 1][:, cx] + fx * d[cy + 1][:, cx + 1]
        out.append(((64 - fy) * top + fy * bottom + 2048) >> 12)
    return tuple(out)


WARP_TRACKING_KEYS = ("tiles", "in_reach", "tracked", "err_rms")


def warp_tracking(field, origin, region, tile_tables):
    """Whether the output followed a deformation of the input tile by tile: a warp row's "tracking" dict (WARP_TRACKING_KEYS) from the
    tile tables (tiles_y, tiles_x, S, S) of its DIRECT displacement comparison over `region` = (ax, ay, bx, by, w, h) of the output
    plane, whose pixel (x, y) sits at grid coordinate (x + ox, y + oy), origin = (ox, oy). Per 64 x 64 tile of the region (the last
    ones ragged) the expected shift is the exact mean over the tile's pixels of (s_0, s_1) / 256 (warp_shifts; an integer sum over
    256 * pixels) and the measured shift the tile's argmin by the tables' tie rule (_displacement_argmin). A tile is in reach when its
    expected shift, rounded half away from zero, lies within the tables' radius on both axes. "tiles": their number; "in_reach": those
    in reach; "tracked": those in reach whose measured shift equals the rounded expected one on both axes; "err_rms": the rms over
    the tiles in reach of the distance between the measured and the expected shift, in pixels (None without a tile in reach). Exact
    integers in, one function on every path: the dict is equal wherever the tables are."""
    ax, ay, _, _, w, h = (int(v) for v in region)
    ox, oy = (int(v) for v in origin)
    tt = np.asarray(tile_tables)
    t, radius = mp.SIM_TILE, tt.shape[2] // 2
    if tt.ndim != 4 or tt.shape[:2] != ((h + t - 1) // t, (w + t - 1) // t) or tt.shape[2] != tt.shape[3] or tt.shape[2] % 2 != 1:
        raise ValueError("expected the (tiles_y, tiles_x, S, S) tile tables of a %d x %d region, got %r" % (w, h, tt.shape))
    s = warp_shifts(field, ax + ox + np.arange(w), ay + oy + np.arange(h))

    def nearest(num, den):   # num / den rounded half away from zero
        q = (2 * abs(num) + den) // (2 * den)
        return q if num >= 0 else -q

    in_reach = tracked = 0
    sq = 0.0
    for ty in range(tt.shape[0]):
        for tx in range(tt.shape[1]):
            tile = [c[ty * t:ty * t + t, tx * t:tx * t + t] for c in s]
            den = mp.WARP_UNIT * tile[0].size
            sx, sy = int(tile[0].sum()), int(tile[1].sum())
            ex, ey = nearest(sx, den), nearest(sy, den)
            if max(abs(ex), abs(ey)) > radius:
                continue
            in_reach += 1
            y, x = _displacement_argmin(tt[ty, tx])
            tracked += (x - radius, y - radius) == (ex, ey)
            sq += (x - radius - sx / den) ** 2 + (y - radius - sy / den) ** 2
    return {"tiles": tt.shape[0] * tt.shape[1], "in_reach": in_reach, "tracked": tracked, "err_rms": math.sqrt(sq / in_reach) if in_reach else None}


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


# ---- contrast-detail: inserted discs, measured where they lie (not in the reference's script) ------------------------------------------
# Every other relation of the study perturbs the whole frame and asks how much the output changed. A contrast-detail phantom, discs of
# graded size and contrast, asks what MUSICA exists to answer: does a small low-contrast object of the raw image come out visible, and
# equally so wherever it lies? A detail is (x, y, r, c): an integer pixel centre, a radius 1 <= r <= DETAIL_MAX_RADIUS and a contrast
# 1 <= |c| <= DETAIL_MAX_CONTRAST in 1 / 1024 of the pixel's value. With d2 = (px - x)^2 + (py - y)^2 its zones are the disc
# d2 <= r^2, the ring (r + 2)^2 <= d2 <= (2r + 2)^2 and the box |px - x|, |py - y| <= Ro = 2r + 2 of side 4r + 5. The boxes of a list
# lie inside the plane and are pairwise disjoint (processing.detail_list), so a pixel belongs to at most one disc and one box and
# nothing depends on the list's order. These functions are the contract of musica_alter_details and musica_sim_details
# (include/musica.h), which are bit-identical to them.

def detail_zones(r):
    """(disc, ring): the boolean masks of a radius-r detail's two zones over its (4r + 5)^2 box, from the integer d2."""
    r = int(r)
    ro = 2 * r + 2
    d = np.arange(-ro, ro + 1, dtype=np.int64)
    d2 = d[:, None] ** 2 + d[None, :] ** 2
    return d2 <= r * r, (d2 >= (r + 2) ** 2) & (d2 <= ro * ro)


def insert_details(image, details):
    """The square 2-D uint16 plane with the discs of `details` (processing.detail_list for its side, else ValueError before any work)
    inserted: inside each disc
        out = min((v * (1024 - c) + 512) >> 10, 65535)
    and every other pixel copied. c > 0 attenuates, as an absorbing object does; c < 0 brightens, as a void does. ONE rounding, halves
    up; the largest intermediate is 65535 * 1536 + 512 < 2^32. With |c| <= 512 a non-zero pixel stays non-zero: v >= 1 gives at least
    (512 + 512) >> 10 = 1. Zeros trigger the early exits of the noise and gradation histograms, so an insertion never creates one. The
    boxes are disjoint, so a pixel belongs to at most one disc and the result does not depend on the list's order."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("insert_details needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    details = mp.detail_list(details, image.shape[0])
    out = image.copy()
    for x, y, r, c in details:
        ro = 2 * r + 2
        disc = detail_zones(r)[0]
        box = out[y - ro:y + ro + 1, x - ro:x + ro + 1]      # a view: the disc's pixels are rewritten in place
        v = box[disc].astype(np.uint64)
        box[disc] = np.minimum((v * np.uint64(1024 - c) + np.uint64(512)) >> np.uint64(10), np.uint64(65535)).astype(np.uint16)
    return out


def detail_statistics(a, b, details):
    """The exact sums of every detail of `details` (in the planes' coordinates; c is not looked at) over two square uint8 planes of equal
    shape: a list of dicts of Python ints, "disc" and "ring" each with n, sum_a, sum_b, sum_aa, sum_bb, sum_ab over the zone, and
    box_ssd = sum over the box of (a - b)^2 with box_pixels = (4r + 5)^2: what musica_sim_details returns."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != a.shape[1] or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("detail_statistics needs two square 2-D uint8 planes of equal shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    details = mp.detail_list(details, a.shape[0], with_contrast=False)
    out = []
    for x, y, r, _ in details:
        ro = 2 * r + 2
        pa = a[y - ro:y + ro + 1, x - ro:x + ro + 1].astype(np.int64)
        pb = b[y - ro:y + ro + 1, x - ro:x + ro + 1].astype(np.int64)
        d = {}
        for zone, mask in zip(mp.DETAIL_ZONES, detail_zones(r)):
            za, zb = pa[mask], pb[mask]
            d[zone] = {"n": int(mask.sum()), "sum_a": int(za.sum()), "sum_b": int(zb.sum()), "sum_aa": int((za * za).sum()),
                       "sum_bb": int((zb * zb).sum()), "sum_ab": int((za * zb).sum())}
        d["box_ssd"] = int(((pa - pb) ** 2).sum())
        d["box_pixels"] = int(pa.size)
        out.append(d)
    return out


DETAIL_KEYS = ("contrast", "halo", "texture", "cnr", "rose", "local_mse")   # detail_summary's numbers of one detail
DETAIL_NOISE_FLOOR = 1.0 / math.sqrt(12.0)                                  # the rms of 8-bit quantisation


def detail_summary(stats):
    """What the study reports of each detail, from detail_statistics' (or musica_sim_details') exact integers: one function for every
    study path, so the paths agree to the last bit. Per detail, in f64 (each quotient of two integers is one correctly rounded division):
        contrast   (mean_disc a - mean_ring a) - (mean_disc b - mean_ring b): the anatomy's own disc - ring difference is removed
        halo       mean_ring (a - b) = (sum_a - sum_b) / n over the ring: the rebound around the detail
        texture    sqrt(max(var_ring b, 0)), the population variance (n sum_bb - sum_b^2) / n^2
        cnr        contrast / max(texture, 1 / sqrt(12)): the floor is the 8-bit quantisation noise
        rose       cnr * sqrt(n_disc)
        local_mse  box_ssd / box_pixels
    No visibility threshold is fixed here: these are findings."""
    out = []
    for s in stats:
        d, g = s["disc"], s["ring"]
        contrast = (d["sum_a"] / d["n"] - g["sum_a"] / g["n"]) - (d["sum_b"] / d["n"] - g["sum_b"] / g["n"])
        texture = math.sqrt(max((g["n"] * g["sum_bb"] - g["sum_b"] * g["sum_b"]) / (g["n"] * g["n"]), 0.0))
        cnr = contrast / max(texture, DETAIL_NOISE_FLOOR)
        out.append({"contrast": contrast, "halo": (g["sum_a"] - g["sum_b"]) / g["n"], "texture": texture, "cnr": cnr,
                    "rose": cnr * math.sqrt(d["n"]), "local_mse": s["box_ssd"] / s["box_pixels"]})
    return out


DETAIL_ROW_KEYS = ("contrast", "cnr", "rose", "halo")     # what a cd_ row's "details" gathers per radius
DETAIL_ROW_STATS = ("mean", "min", "max", "std")


def detail_row(details, stats, sq_diff_sum, pixels, tables=False):
    """A cd_ row's "details" value from the row's details (their radii), their exact sums and the full frame's exact sum of squared
    differences over `pixels` pixels: {"radii": {r: {"count", and for each of DETAIL_ROW_KEYS its mean, min, max and population std over
    the positions of the radius-r details}}, in ascending r, "outside_mse": (sq_diff_sum - sum box_ssd) / (pixels - sum box_pixels), the
    locality statistic (what changed away from every detail's neighbourhood)}, with tables=True also "per_detail": the (x, y, r, c) and
    detail_summary's numbers of every detail, in the list's order."""
    summary = detail_summary(stats)
    radii = {}
    for r in sorted(set(d[2] for d in details)):
        group = [s for d, s in zip(details, summary) if d[2] == r]
        radii[r] = {"count": len(group)}
        for k in DETAIL_ROW_KEYS:
            v = [s[k] for s in group]
            mean = math.fsum(v) / len(v)
            radii[r][k] = {"mean": mean, "min": min(v), "max": max(v), "std": math.sqrt(math.fsum((x - mean) * (x - mean) for x in v) / len(v))}
    boxes, inside = sum(s["box_ssd"] for s in stats), sum(s["box_pixels"] for s in stats)
    outside = int(pixels) - inside    # 0 only when one box is the whole plane
    out = {"radii": radii, "outside_mse": (int(sq_diff_sum) - boxes) / outside if outside else 0.0}
    if tables:
        out["per_detail"] = [dict(s, x=d[0], y=d[1], r=d[2], c=d[3]) for d, s in zip(details, summary)]
    return out


# ---- point response: defect pixels and clusters, the response stacked where they lie (not in the reference's script) ------------------
# The impulse of the classical measurements. A point is (x, y, R, s, c, group): an integer pixel centre, the half-side POINT_MIN_RADIUS
# <= R <= POINT_MAX_RADIUS of its window |dx|, |dy| <= R (side S = 2R + 1; one R for the whole list), the cluster size 1 <= s <=
# POINT_MAX_SIZE (along each axis the offsets -((s - 1) // 2) .. s // 2: one pixel, x .. x + 1, x - 1 .. x + 1, all inside the core
# |dx|, |dy| <= 1), the contrast POINT_MIN_CONTRAST <= c <= POINT_MAX_CONTRAST, c != 0, in 1 / 1024 of the pixel's value, and a group
# below POINT_MAX_GROUPS. The windows of a list lie inside the plane and are pairwise disjoint (processing.point_list), so nothing
# depends on the list's order. Everything up to point_summary is integer: these functions are the contract of musica_alter_points and
# musica_sim_points (include/musica.h), which are bit-identical to them.

def point_cluster(s):
    """(lo, hi): the first and last offset, along each axis, of a cluster of size s: (0, 0), (0, 1), (-1, 1) for s = 1, 2, 3."""
    s = int(s)
    return -((s - 1) // 2), s // 2


def insert_points(image, points):
    """The square 2-D uint16 plane with the clusters of `points` (processing.point_list for its side, else ValueError before any work)
    altered: inside each cluster
        out = min((v * (1024 - c) + 512) >> 10, 65535)
    and every other pixel copied. ONE rounding, halves up; c = 1024 is a dead element (0), c = -64512 multiplies by 64 and saturates
    everything above 1023 counts (a hot element); the largest intermediate is 65535 * 65536 + 512 < 2^32. UNLIKE insert_details an
    insertion with c > 512 can create zeros (v = 1, c = 513 gives 0), which trigger the early exits of the noise and gradation
    histograms: that is what a dead element does to them, and part of what the rows measure. The windows are disjoint, so a pixel
    belongs to at most one cluster and the result does not depend on the list's order."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("insert_points needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    points = mp.point_list(points, image.shape[0])
    out = image.copy()
    for x, y, _, s, c, _ in points:
        lo, hi = point_cluster(s)
        v = out[y + lo:y + hi + 1, x + lo:x + hi + 1].astype(np.uint64)
        out[y + lo:y + hi + 1, x + lo:x + hi + 1] = np.minimum((v * np.uint64(1024 - c) + np.uint64(512)) >> np.uint64(10), np.uint64(65535)).astype(np.uint16)
    return out


def point_statistics(a, b, points, groups=None):
    """The exact sums of the points of `points` (in the planes' coordinates; c is not looked at) over two square uint8 planes of equal
    shape, what musica_sim_points returns: {"points": per point a dict of the Python ints core_sum_a, core_sum_b (over the 3 x 3 core),
    win_sum_a, win_sum_b, win_ssd = sum of (a - b)^2 (over the window) and win_pixels = S^2; "groups": per group 0 .. groups - 1
    (processing.point_groups: by default 1 + the largest group) a dict of "count", the group's points, and the stack, the (S, S) int64
    arrays sum_a, sum_b and ssd indexed [dy + R, dx + R]: over the group's points p the sums of a(p + o), b(p + o) and (a - b)^2(p + o).
    A group without points is all zero."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != a.shape[1] or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("point_statistics needs two square 2-D uint8 planes of equal shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    points = mp.point_list(points, a.shape[0], with_contrast=False)
    groups = mp.point_groups(points, groups)
    r = points[0][2]
    side = 2 * r + 1
    stacks = [dict({"count": 0}, **{k: np.zeros((side, side), dtype=np.int64) for k in mp.POINT_STACKS}) for _ in range(groups)]
    per_point = []
    for x, y, _, _, _, g in points:
        pa = a[y - r:y + r + 1, x - r:x + r + 1].astype(np.int64)
        pb = b[y - r:y + r + 1, x - r:x + r + 1].astype(np.int64)
        dd = (pa - pb) ** 2
        per_point.append({"core_sum_a": int(pa[r - 1:r + 2, r - 1:r + 2].sum()), "core_sum_b": int(pb[r - 1:r + 2, r - 1:r + 2].sum()),
                          "win_sum_a": int(pa.sum()), "win_sum_b": int(pb.sum()), "win_ssd": int(dd.sum()), "win_pixels": side * side})
        stack = stacks[g]
        stack["count"] += 1
        stack["sum_a"] += pa
        stack["sum_b"] += pb
        stack["ssd"] += dd
    return {"points": per_point, "groups": stacks}


POINT_KEYS = ("count", "peak", "gain", "volume", "fwhm", "rebound", "rebound_radius", "reach", "anisotropy", "spread", "level_slope", "level_r")   # point_summary's scalars; "radial" beside them
POINT_CSV_HEADER = ['raw file', 'alteration', 'group'] + [k.replace('_', ' ') for k in POINT_KEYS] + ['outside mse']   # point_response.csv


def _point_response(count, sum_a, sum_b, ssd, cores, contrast):
    """point_summary's numbers of one stack of `count` points: the (S, S) int64 arrays, the points' (core_sum_a, core_sum_b) and the
    contrast the gain is taken against."""
    out = dict.fromkeys(POINT_KEYS)
    out["count"], out["radial"] = int(count), None
    if not count:
        return out
    side = sum_a.shape[0]
    r = side // 2
    h = (sum_a - sum_b).astype(np.float64) / float(count)
    d = np.arange(-r, r + 1, dtype=np.int64)
    dy, dx = d[:, None] + 0 * d[None, :], 0 * d[:, None] + d[None, :]
    d2 = dx * dx + dy * dy
    inside = d2 <= r * r
    rho = np.array([[math.isqrt(int(v)) for v in row] for row in d2], dtype=np.int64)
    peak = float(h[r, r])
    radial = [math.fsum(h[inside & (rho == k)].tolist()) / int((inside & (rho == k)).sum()) for k in range(r + 1)]
    h2 = h * h
    energy = [math.fsum(h2[inside & (rho == k)].tolist()) for k in range(r + 1)]
    total = math.fsum(energy)
    reach = next(k for k in range(r + 1) if math.fsum(energy[:k + 1]) >= 0.9 * total)
    all2 = math.fsum(h2.ravel().tolist())
    moment = math.fsum((h2 * d2).ravel().tolist())
    out.update(peak=peak, gain=peak * 1024.0 / contrast if contrast else None, volume=math.fsum(h.ravel().tolist()), radial=radial, reach=reach,
               anisotropy=(math.fsum((h2 * (dx * dx)).ravel().tolist()) - math.fsum((h2 * (dy * dy)).ravel().tolist())) / moment if moment else 0.0,
               spread=math.sqrt(max(math.fsum((ssd.astype(np.float64) / float(count) - h2).ravel().tolist()), 0.0) / all2) if all2 else None)
    if peak != 0.0:
        rel = [v / peak for v in radial]
        k = next((k for k in range(1, r + 1) if rel[k] < 0.5), None)
        if k is not None:
            out["fwhm"] = 2.0 * ((k - 1) + (rel[k - 1] - 0.5) / (rel[k - 1] - rel[k]))
        k = min(range(r + 1), key=lambda k: rel[k])
        out["rebound"], out["rebound_radius"] = (rel[k], k) if rel[k] < 0.0 else (0.0, None)
    if len(cores) >= 2:
        x = [cb / 9.0 for _, cb in cores]
        y = [float(ca - cb) for ca, cb in cores]
        mx, my = math.fsum(x) / len(x), math.fsum(y) / len(y)
        sxx = math.fsum((u - mx) * (u - mx) for u in x)
        syy = math.fsum((v - my) * (v - my) for v in y)
        sxy = math.fsum((u - mx) * (v - my) for u, v in zip(x, y))
        if sxx > 0.0:
            out["level_slope"] = sxy / sxx
            if syy > 0.0:
                out["level_r"] = sxy / math.sqrt(sxx * syy)
    return out


def point_summary(stats, points):
    """What the study reports of a point list, from point_statistics' (or musica_sim_points') exact integers: one function for every
    study path, so the paths agree to the last bit. {"groups": [one dict per group], "all": the same over all the points (the groups'
    stacks added)}. With h(o) = (sum_a - sum_b)(o) / count, the mean response at offset o = (dx, dy), in f64 (sums by math.fsum):
        count           the points
        peak            h(0, 0)
        gain            peak * 1024 / c, signed: c is the contrast of the first point of the group (of the list, for "all")
        volume          sum of h over the window
        radial          the mean of h per class rho = floor(sqrt(dx^2 + dy^2)), rho = 0 .. R, over dx^2 + dy^2 <= R^2
        fwhm            twice the radius at which radial / peak first falls below 1 / 2, interpolated linearly between the two classes;
                        None if the peak is 0 or it never does
        rebound         the extreme of radial of the sign opposite to the peak, divided by the peak (so negative; 0.0 where there is none,
                        None if the peak is 0), and rebound_radius, the class where it lies (None where there is none)
        reach           the smallest rho whose classes 0 .. rho hold 90 % of the sum of h^2 within d^2 <= R^2
        anisotropy      (sum h^2 dx^2 - sum h^2 dy^2) / sum h^2 (dx^2 + dy^2) over the window; 0.0 where that is 0 / 0
        spread          sqrt(sum_o (ssd(o) / count - h(o)^2) / sum_o h(o)^2): how much the response differs from position to position;
                        None where h is 0 everywhere
        level_slope, level_r   the points' core responses core_sum_a - core_sum_b regressed on their backgrounds core_sum_b / 9: the
                        slope and Pearson's r; None with fewer than two points or without variance
    A group without points has its count 0 and None everywhere else. None of these is asserted anywhere: they are findings."""
    groups = stats["groups"]
    out = []
    for g, stack in enumerate(groups):
        mine = [i for i, p in enumerate(points) if p[5] == g]
        cores = [(stats["points"][i]["core_sum_a"], stats["points"][i]["core_sum_b"]) for i in mine]
        out.append(_point_response(stack["count"], stack["sum_a"], stack["sum_b"], stack["ssd"], cores, points[mine[0]][4] if mine else 0))
    cores = [(s["core_sum_a"], s["core_sum_b"]) for s in stats["points"]]
    whole = _point_response(sum(s["count"] for s in groups), *[sum(np.asarray(s[k], dtype=np.int64) for s in groups) for k in mp.POINT_STACKS], cores, points[0][4])
    return {"groups": out, "all": whole}


def point_row(points, stats, sq_diff_sum, pixels, tables=False):
    """A point_ row's "points" value from the row's points, their exact sums and stacks and the full frame's exact sum of squared
    differences over `pixels` pixels: point_summary's {"groups", "all"} and "outside_mse": (sq_diff_sum - sum win_ssd) / (pixels - sum
    win_pixels), how far beyond R the change reaches (0.0 when the windows are the whole frame); with tables=True also "per_point": the
    (x, y, R, s, c, group) and the exact sums of every point, in the list's order, and "stacks": per group its count and the three
    planes as nested lists of Python ints."""
    out = point_summary(stats, points)
    inside_ssd, inside = sum(s["win_ssd"] for s in stats["points"]), sum(s["win_pixels"] for s in stats["points"])
    outside = int(pixels) - inside
    out["outside_mse"] = (int(sq_diff_sum) - inside_ssd) / outside if outside else 0.0
    if tables:
        out["per_point"] = [dict(s, x=p[0], y=p[1], R=p[2], s=p[3], c=p[4], group=p[5]) for p, s in zip(points, stats["points"])]
        out["stacks"] = [dict({"count": int(g["count"])}, **{k: np.asarray(g[k]).astype(np.int64).tolist() for k in mp.POINT_STACKS}) for g in stats["groups"]]
    return out


# ---- edge response: slanted edges, the edge-spread function binned where they lie (not in the reference's script) ---------------------
# MTF, NPS and contrast-detail are the classic triad; the ensemble gives the NPS, the cd_ rows the contrast-detail curve, and this is the
# third: how MUSICA renders an edge (ISO 12233 / IEC 62220 slanted edge). An edge is (x, y, h, p, q, o, c): an integer pixel centre, a
# half-side EDGE_MIN_HALF <= h <= EDGE_MAX_HALF, a rational slope p / q (1 <= p < q, EDGE_MIN_Q <= q <= EDGE_MAX_Q, lowest terms), an
# orientation o = 0 .. 3 and a contrast 1 <= |c| <= EDGE_MAX_CONTRAST in 1 / 1024 of the pixel's value. With dx = px - x, dy = py - y
# the profile coordinate u and the along-edge coordinate v are (dx, dy), (dy, dx), (-dx, dy), (-dy, dx) for o = 0, 1, 2, 3 and the
# signed numerator is s = q u - p v: s / q is the pixel's distance from the edge along the profile axis, in pixels. The plate
# |dx|, |dy| <= 2h (side 4h + 1) is what gets inserted, the region |dx|, |dy| <= h (side 2h + 1) what gets measured: the region keeps
# h pixels of the plate around it, so the processor's response to the plate's own border stays out of the profile. The plates of a list
# lie inside the plane and are pairwise disjoint (processing.edge_list), so nothing depends on the list's order. Everything up to
# edge_summary is integer: these functions are the contract of musica_alter_edges and musica_sim_edges (include/musica.h), which are
# bit-identical to them.

def edge_numerators(h, p, q, o, reach):
    """s = q u - p v of every pixel of the square |dx|, |dy| <= reach about an edge's centre, an int64 array indexed [dy + reach,
    dx + reach]. `h` is not looked at."""
    d = np.arange(-int(reach), int(reach) + 1, dtype=np.int64)
    dy, dx = d[:, None], d[None, :]
    u, v = ((dx, dy), (dy, dx), (-dx, dy), (-dy, dx))[int(o)]
    return int(q) * u - int(p) * v + 0 * (dx + dy)


def insert_edges(image, edges):
    """The square 2-D uint16 plane with the plates of `edges` (processing.edge_list for its side, else ValueError before any work)
    inserted: inside each plate, with m = clamp(2s + q, 0, 2q),
        out = min((v * (2048 q - c m) + 1024 q) // (2048 q), 65535)
    and every other pixel copied. m / 2q is the part of the pixel's one-pixel box aperture along the profile axis that the absorber
    (s > 0) covers, so the edge is an area-sampled ideal step, with ONE rounding, halves up. m = 0 gives exactly v, m = 2q exactly
    detail_pixel's min((v (1024 - c) + 512) >> 10, 65535); the largest intermediate is 65535 * (2048 * 16 + 512 * 32) + 16384 < 2^32.
    As for the details a non-zero pixel stays non-zero."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("insert_edges needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    edges = mp.edge_list(edges, image.shape[0])
    out = image.copy()
    for x, y, h, p, q, o, c in edges:
        m = np.clip(2 * edge_numerators(h, p, q, o, 2 * h) + q, 0, 2 * q)
        plate = out[y - 2 * h:y + 2 * h + 1, x - 2 * h:x + 2 * h + 1]      # a view: the plate is rewritten in place
        plate[...] = np.minimum((plate.astype(np.int64) * (2048 * q - c * m) + 1024 * q) // (2048 * q), 65535).astype(np.uint16)
    return out


def edge_statistics(a, b, edges):
    """The exact edge-spread tables of every edge of `edges` (in the planes' coordinates; c is not looked at) over two square uint8
    planes of equal shape: what musica_sim_edges returns. Every pixel of the region falls in bin k = floor(4 s / q) (a floor division,
    negative s included): the profile oversampled four times. With B = ceil(4 (q + p) h / q) the table has bins = 2B + 1 entries
    (processing.edge_bins) and bin k is stored at index k + B. One dict per edge: the ints h, p, q, bins, the uint32 arrays n, sum_a,
    sum_b, sum_aa (the pixels of each bin, their sums over a and b, the sum of a^2), roi_ssd = the sum over the region of (a - b)^2 and
    roi_pixels = (2h + 1)^2. A bin receives at most one pixel per line of the region across the profile, so n <= 2h + 1 and every sum
    fits uint32; every bin -C <= k < C, C = floor(4 (q - p) h / q), is non-empty."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != a.shape[1] or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("edge_statistics needs two square 2-D uint8 planes of equal shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    edges = mp.edge_list(edges, a.shape[0], with_contrast=False)
    out = []
    for x, y, h, p, q, o, _ in edges:
        bins = mp.edge_bins(h, p, q)
        k = ((4 * edge_numerators(h, p, q, o, h)) // q + bins // 2).ravel()
        pa = a[y - h:y + h + 1, x - h:x + h + 1].astype(np.int64).ravel()
        pb = b[y - h:y + h + 1, x - h:x + h + 1].astype(np.int64).ravel()
        d = {"h": h, "p": p, "q": q, "bins": bins, "roi_ssd": int(((pa - pb) ** 2).sum()), "roi_pixels": int(pa.size)}
        for key, w in zip(mp.EDGE_SUMS, (np.ones_like(pa), pa, pb, pa * pa)):
            d[key] = np.bincount(k, weights=w, minlength=bins).astype(np.uint32)   # exact: every sum is below 2^53
        out.append(d)
    return out


EDGE_SIDES = ("a", "b", "d")                # the three edge-spread functions of an edge: of side a, of side b, of a - b
EDGE_KEYS = ("low", "high", "step", "rise", "overshoot", "undershoot", "mtf50", "mtf10", "mtf_peak", "mtf_peak_f")   # edge_profile's numbers
EDGE_FFT = 4096                             # the zero-padded length of the line-spread function's transform: a power of two above EDGE_BINS_MAX


def edge_pitch(p, q):
    """The distance in pixels along the edge's normal between two bins of the four-times oversampled profile: 1/4 q / sqrt(p^2 + q^2)."""
    return 0.25 * q / math.sqrt(p * p + q * q)


def edge_mtf(esf, pitch):
    """(f, mtf): the edge MTF of an edge-spread function sampled every `pitch` pixels, at the frequencies f_j = j / (EDGE_FFT pitch)
    <= 0.5 cycles / pixel (up to the pixel grid's Nyquist frequency), or (f, None) when the windowed line-spread function sums to 0.
    The line-spread function is the difference l_i = e_(i+1) - e_i of the M + 1 samples, windowed with the Hann window
    w_i = 1/2 - 1/2 cos(2 pi (i + 1/2) / M) (centred on the profile's centre, where the edge lies; no sample is weighted 0),
    zero-padded to EDGE_FFT and transformed; |L(f)| is divided by |L(0)|, so mtf[0] is exactly 1, and by sinc^2(f pitch)
    (sinc(x) = sin(pi x) / (pi x)): once for the bin, which averages the profile over a box one pitch wide, and once for the
    difference, which is the derivative convolved with the same box."""
    e = np.asarray(esf, dtype=np.float64)
    f = np.arange(int(math.floor(0.5 * EDGE_FFT * pitch)) + 1, dtype=np.float64) / (EDGE_FFT * pitch)
    if e.size < 3:
        return f, None
    m = e.size - 1
    lsf = np.diff(e) * (0.5 - 0.5 * np.cos(2.0 * math.pi * (np.arange(m) + 0.5) / m))
    spectrum = np.abs(np.fft.rfft(lsf, EDGE_FFT))[:f.size]
    if spectrum[0] == 0.0:
        return f, None
    return f, (spectrum / spectrum[0]) / np.sinc(f * pitch) ** 2


def _crossing(x, y, level, rising):
    """The first x, scanning up, at which the piecewise-linear y crosses `level` (upwards if `rising`, else downwards), linearly
    interpolated between the two samples; None where it does not."""
    for i in range(1, len(y)):
        lo, hi = (y[i - 1], y[i]) if rising else (-y[i - 1], -y[i])
        t = level if rising else -level
        if lo < t <= hi:
            return float(x[i - 1] + (x[i] - x[i - 1]) * (t - lo) / (hi - lo))
    return None


def edge_profile(esf, pitch):
    """The numbers (EDGE_KEYS) of one edge-spread function, the 2C central bins of a table in ascending k, sampled every `pitch` pixels:
        low, high   the plateau means: of the first and of the last W = max(C // 4, 1) samples (math.fsum / W)
        step        high - low, signed: which side comes out brighter is the processor's business
        rise        with e = (esf - low) / step, the distance in pixels along the edge's normal between the first upward crossing of
                    0.1 and the first upward crossing of 0.9 at or behind it, both interpolated linearly between samples
        overshoot   max(max e - 1, 0), undershoot max(-min e, 0): fractions of the step, the rebound past the last plateau and
                    before the first (in the direction of ascending k, whatever the step's sign)
        mtf50, mtf10   the lowest frequency in cycles / pixel at which edge_mtf falls through 0.5 and 0.1, interpolated linearly
        mtf_peak, mtf_peak_f   the largest value of edge_mtf up to 0.5 cycles / pixel (an enhancement lifts it above 1) and where
    rise, overshoot and undershoot are None for a step of 0, the four MTF numbers where edge_mtf has none, a crossing where the
    curve does not cross."""
    e = [float(v) for v in esf]
    w = max(len(e) // 8, 1)
    low, high = math.fsum(e[:w]) / w, math.fsum(e[-w:]) / w
    out = dict.fromkeys(EDGE_KEYS)
    out.update(low=low, high=high, step=high - low)
    if out["step"] != 0.0:
        n = [(v - low) / out["step"] for v in e]
        pos = [i * pitch for i in range(len(n))]
        x10 = _crossing(pos, n, 0.1, True)
        first = next((i for i in range(1, len(n)) if x10 is not None and pos[i] >= x10), None)
        x90 = None if first is None else _crossing([x10] + pos[first:], [0.1] + n[first:], 0.9, True)
        out.update(rise=None if x90 is None else x90 - x10, overshoot=max(max(n) - 1.0, 0.0), undershoot=max(-min(n), 0.0))
    f, mtf = edge_mtf(e, pitch)
    if mtf is not None:
        peak = int(np.argmax(mtf))
        out.update(mtf50=_crossing(f, mtf, 0.5, False), mtf10=_crossing(f, mtf, 0.1, False), mtf_peak=float(mtf[peak]), mtf_peak_f=float(f[peak]))
    return out


def edge_central(h, p, q):
    """C = floor(4 (q - p) h / q): the bins -C <= k < C of an edge's table are non-empty whatever the orientation (>= 2 for h >= 8)."""
    return (4 * (q - p) * h) // q


def edge_summary(stats):
    """What the study reports of each edge, from edge_statistics' (or musica_sim_edges') exact integers: one function for every study
    path, so the paths agree to the last bit. Per edge, in f64 and from the central bins -C .. C - 1 only (edge_central): "esf", the
    three edge-spread functions as lists, a = sum_a / n, b = sum_b / n and d = (sum_a - sum_b) / n (each one correctly rounded division
    of two integers; d is the response to the edge alone, the anatomy under it removed) with "k0" = -C and "pitch" = edge_pitch(p, q);
    and under "a", "b" and "d" edge_profile's numbers of each. No threshold is fixed here: these are findings."""
    out = []
    for s in stats:
        c, big = edge_central(s["h"], s["p"], s["q"]), s["bins"] // 2
        n, sa, sb = ([int(v) for v in s[k][big - c:big + c]] for k in ("n", "sum_a", "sum_b"))
        esf = {"a": [x / m for x, m in zip(sa, n)], "b": [x / m for x, m in zip(sb, n)], "d": [(x - y) / m for x, y, m in zip(sa, sb, n)]}
        pitch = edge_pitch(s["p"], s["q"])
        d = {side: edge_profile(esf[side], pitch) for side in EDGE_SIDES}
        d["esf"] = dict(esf, k0=-c, pitch=pitch)
        out.append(d)
    return out


EDGE_ROW_KEYS = ("step", "rise", "overshoot", "undershoot", "mtf50", "mtf_peak")   # what an edge_ row's "edges" gathers, of the d profile
EDGE_ROW_STATS = ("min", "mean", "max", "count")


def _edge_spread(summary):
    out = {"edges": len(summary)}
    for k in EDGE_ROW_KEYS:
        v = [s["d"][k] for s in summary if s["d"][k] is not None]
        out[k] = {"min": min(v), "mean": math.fsum(v) / len(v), "max": max(v), "count": len(v)} if v else {"min": None, "mean": None, "max": None, "count": 0}
    return out


def edge_row(edges, stats, sq_diff_sum, pixels, tables=False):
    """An edge_ row's "edges" value from the row's edges, their exact tables and the full frame's exact sum of squared differences over
    `pixels` pixels: {"all": spread, "orientations": {o: spread}, "halves": {h: spread}, in ascending o and h, "outside_mse":
    (sq_diff_sum - sum roi_ssd) / (pixels - sum roi_pixels), the change away from every region}. A spread is {"edges": the group's
    size, and for each of EDGE_ROW_KEYS (of the a - b profile) its min, mean, max over the edges that have the number and their
    count}. With tables=True also "per_edge": the (x, y, h, p, q, o, c) and edge_summary's dict of every edge, the three
    edge-spread functions included, in the list's order."""
    summary = edge_summary(stats)
    out = {"all": _edge_spread(summary)}
    for name, at in (("orientations", 5), ("halves", 2)):
        out[name] = {g: _edge_spread([s for e, s in zip(edges, summary) if e[at] == g]) for g in sorted(set(e[at] for e in edges))}
    rois, inside = sum(s["roi_ssd"] for s in stats), sum(s["roi_pixels"] for s in stats)
    outside = int(pixels) - inside
    out["outside_mse"] = (int(sq_diff_sum) - rois) / outside if outside else 0.0
    if tables:
        out["per_edge"] = [dict(s, x=e[0], y=e[1], h=e[2], p=e[3], q=e[4], o=e[5], c=e[6]) for e, s in zip(edges, summary)]
    return out


# ---- grating response: sine patches, the region folded by phase where they lie (not in the reference's script) -------------------------
# What defines a multi-scale contrast equaliser is its gain as a function of spatial frequency and of amplitude; the edge rows give one
# broadband MTF per contrast and the discs mix all frequencies of their size. The classical test object is the line-pair / sine grating
# patch. A grating is (x, y, h, ux, uy, T, wave): an integer pixel centre, a half-side GRATING_MIN_HALF <= h <= GRATING_MAX_HALF, a wave
# vector (ux, uy) with |ux|, |uy| <= GRATING_MAX_U, not both 0 and coprime, a period 2 <= T <= min(GRATING_MAX_PERIOD, h) with
# 2 |ux| <= T and 2 |uy| <= T (no aliasing along either axis; |u| / T cycles per pixel along u), and a wave of T integers
# |w| <= GRATING_MAX_CONTRAST in 1 / 1024 of the pixel's value. With dx = px - x, dy = py - y the phase of a pixel is
# k = (ux dx + uy dy) mod T, in 0 .. T - 1. The plate |dx|, |dy| <= 2h is what gets inserted, the region |dx|, |dy| <= h what gets
# measured, as for the edges; the plates of a list lie inside the plane and are pairwise disjoint (processing.grating_list). Everything
# up to grating_summary is integer: these functions are the contract of musica_alter_gratings and musica_sim_gratings
# (include/musica.h), which are bit-identical to them. The device contract starts from the integer wave table: the cosine of
# grating_wave is the study's choice, not the library's.

def grating_phases(ux, uy, period, reach):
    """k = (ux dx + uy dy) mod T, in 0 .. T - 1, of every pixel of the square |dx|, |dy| <= reach about a grating's centre, an int64
    array indexed [dy + reach, dx + reach]."""
    d = np.arange(-int(reach), int(reach) + 1, dtype=np.int64)
    return (int(ux) * d[None, :] + int(uy) * d[:, None]) % int(period)


def grating_wave(period, contrast):
    """The study's wave table: w[k] = floor(c cos(2 pi k / T) + 1/2) for k = 0 .. T - 1, a cosine of amplitude c / 1024 that attenuates
    most at phase 0, as a tuple of ints. Where 12 k / T is an integer and the cosine is rational (0, +-1/2, +-1: the even multiples of
    pi / 6 and the odd multiples of pi / 2) the exact value is substituted and the rounding done in integers, floor((2 c cos + 1) / 2).
    This makes the table the same on every libm: floor(z + 1/2) depends on the last bits of z = c cos only next to a half-integer z, and
    a z that IS a half-integer needs a rational cosine, (2j + 1) / (2c); by Niven's theorem the only rational cosines of rational
    multiples of pi are 0, +-1/2 and +-1, all substituted here. For even c they give the integers 0, +-c/2, +-c, so there are no ties
    at all; for odd c the tie at +-1/2 is rounded up, exactly. (Everywhere else z stays at least 1e-6 from a half-integer over the
    whole domain T <= GRATING_MAX_PERIOD, c <= GRATING_MAX_CONTRAST, ten orders above a libm's error: tests/test_grating_restatement.py.)"""
    t, c = int(period), int(contrast)
    if not (2 <= t <= mp.GRATING_MAX_PERIOD and abs(c) <= mp.GRATING_MAX_CONTRAST):
        raise ValueError("grating_wave needs 2 <= T <= %d and |c| <= %d, got %r, %r" % (mp.GRATING_MAX_PERIOD, mp.GRATING_MAX_CONTRAST, period, contrast))
    twice = {0: 2, 2: 1, 3: 0, 4: -1, 6: -2, 8: -1, 9: 0, 10: 1}     # 2 cos(m pi / 6) where it is rational
    out = []
    for k in range(t):
        m = 12 * k // t if (12 * k) % t == 0 else None
        out.append((c * twice[m] + 1) // 2 if m in twice else int(math.floor(c * math.cos(2.0 * math.pi * k / t) + 0.5)))
    return tuple(out)


def insert_gratings(image, gratings):
    """The square 2-D uint16 plane with the plates of `gratings` (processing.grating_list for its side, else ValueError before any
    work) inserted: inside each plate
        out = min((v * (1024 - wave[k]) + 512) >> 10, 65535)
    and every other pixel copied: ONE rounding, halves up. wave[k] = 0 gives exactly v; the largest intermediate is 65535 * 1536 + 512
    < 2^32; a non-zero pixel stays non-zero (v * 512 + 512 >= 1024 for v >= 1)."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("insert_gratings needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    gratings = mp.grating_list(gratings, image.shape[0])
    out = image.copy()
    for x, y, h, ux, uy, t, wave in gratings:
        w = np.array(wave, dtype=np.int64)[grating_phases(ux, uy, t, 2 * h)]
        plate = out[y - 2 * h:y + 2 * h + 1, x - 2 * h:x + 2 * h + 1]      # a view: the plate is rewritten in place
        plate[...] = np.minimum((plate.astype(np.int64) * (1024 - w) + 512) >> 10, 65535).astype(np.uint16)
    return out


def grating_statistics(a, b, gratings):
    """The exact phase-folded tables of every grating of `gratings` (in the planes' coordinates; the wave is not looked at) over two
    square uint8 planes of equal shape: what musica_sim_gratings returns. Every pixel of the region falls in bin k, its phase. One dict
    per grating: the ints h, ux, uy, T, the uint32 arrays n, sum_a, sum_b, sum_aa of T entries (the pixels of each bin, their sums over
    a and b, the sum of a^2), roi_ssd = the sum over the region of (a - b)^2 and roi_pixels = (2h + 1)^2.
    Every bin is non-empty: dx and dy each run over S = 2h + 1 >= 2T + 1 consecutive values, so ux dx reaches every multiple of
    gcd(ux, T) mod T and uy dy every multiple of gcd(uy, T), together every multiple of gcd(ux, uy, T) = 1. A bin holds at most
    ceil(S / 2) S pixels: one of ux, uy is not 0 mod T (2 |u| <= T and gcd(ux, uy) = 1), so along that axis a phase repeats at a
    period of at least 2; S <= 257 gives 33153 pixels and 33153 * 255^2 < 2^32, so every sum fits uint32."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != a.shape[1] or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("grating_statistics needs two square 2-D uint8 planes of equal shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    gratings = mp.grating_list(gratings, a.shape[0], with_wave=False)
    out = []
    for x, y, h, ux, uy, t, _ in gratings:
        k = grating_phases(ux, uy, t, h).ravel()
        pa = a[y - h:y + h + 1, x - h:x + h + 1].astype(np.int64).ravel()
        pb = b[y - h:y + h + 1, x - h:x + h + 1].astype(np.int64).ravel()
        d = {"h": h, "ux": ux, "uy": uy, "T": t, "roi_ssd": int(((pa - pb) ** 2).sum()), "roi_pixels": int(pa.size)}
        for key, w in zip(mp.GRATING_SUMS, (np.ones_like(pa), pa, pb, pa * pa)):
            d[key] = np.bincount(k, weights=w, minlength=t).astype(np.uint32)   # exact: every sum is below 2^53
        out.append(d)
    return out


GRATING_SIDES = ("a", "b", "d")     # the three folded profiles of a grating: of side a, of side b, of a - b
GRATING_HARMONICS = 3               # the harmonics h = 1 .. 3 that grating_summary reports


def grating_harmonic(profile, h):
    """(amplitude, phase) of harmonic h >= 1 of one period m_0 .. m_(T-1) of a profile, or None where 2h > T (the harmonic does not
    exist): X = sum_k m_k e^(-2 pi i h k / T) (math.fsum of the real and of the imaginary parts, the angle reduced in integers,
    2 pi ((h k) mod T) / T), the amplitude (2 / T) |X|, or (1 / T) |X| for the Nyquist harmonic 2h = T, the phase atan2(Im X, Re X):
    m_k = A cos(2 pi h k / T - p) gives (A, -p)."""
    t = len(profile)
    if 2 * h > t:
        return None
    re = math.fsum(v * math.cos(2.0 * math.pi * ((h * k) % t) / t) for k, v in enumerate(profile))
    im = -math.fsum(v * math.sin(2.0 * math.pi * ((h * k) % t) / t) for k, v in enumerate(profile))
    return ((1.0 if 2 * h == t else 2.0) / t) * math.hypot(re, im), math.atan2(im, re)


def grating_summary(stats, gratings):
    """What the study reports of each grating, from grating_statistics' (or musica_sim_gratings') exact integers and the list's waves:
    one function for every study path, so the paths agree to the last bit. Per grating, in f64:
        folded      {"a": sum_a / n, "b": sum_b / n, "d": (sum_a - sum_b) / n}: the three mean profiles over one period, as lists (each
                    one correctly rounded division of two integers; d is the response to the grating alone, the anatomy removed)
        dc          the mean of d over the period (math.fsum / T)
        amplitude, harmonic_phase   lists over h = 1, 2, 3 of grating_harmonic(d, h)'s two numbers, None where 2h > T
        input       the amplitude of the fundamental of wave / 1024: the relative input modulation
        response    amplitude[0]: the fundamental of d, in gray levels
        gain        response / input, gray levels per unit of relative input modulation, comparable across contrasts; None for input 0
        phase       the phase of d's fundamental less the wave's, in (-pi, pi]; None for input 0. The wave ATTENUATES, so an output that
                    is darker where the wave is largest gives +-pi and a processor that inverts the pattern 0.
        thd         sqrt(A2^2 + A3^2) / A1 over the harmonics that exist (T >= 4: A2; T >= 6: A3 as well); None where none exists or
                    A1 = 0
        texture     the pooled within-phase variance of a, sum_k (sum_aa - sum_a^2 / n) / sum_k n
        roi_mse     roi_ssd / roi_pixels
    No threshold is fixed here: these are findings."""
    out = []
    for s, g in zip(stats, gratings):
        n, sa, sb, saa = ([int(v) for v in s[k]] for k in mp.GRATING_SUMS)
        folded = {"a": [x / m for x, m in zip(sa, n)], "b": [x / m for x, m in zip(sb, n)], "d": [(x - y) / m for x, y, m in zip(sa, sb, n)]}
        t = len(n)
        harmonics = [grating_harmonic(folded["d"], h) for h in range(1, GRATING_HARMONICS + 1)]
        d = {"folded": folded, "dc": math.fsum(folded["d"]) / t, "amplitude": [None if v is None else v[0] for v in harmonics],
             "harmonic_phase": [None if v is None else v[1] for v in harmonics]}
        win, wph = grating_harmonic([w / 1024.0 for w in g[6]], 1)
        response = d["amplitude"][0]
        turn = None if win == 0.0 else d["harmonic_phase"][0] - wph
        if turn is not None:
            turn -= 2.0 * math.pi * math.ceil((turn - math.pi) / (2.0 * math.pi))
        higher = [v for v in d["amplitude"][1:] if v is not None]
        d.update(input=win, response=response, gain=None if win == 0.0 else response / win, phase=turn,
                 thd=math.sqrt(math.fsum(v * v for v in higher)) / response if higher and response != 0.0 else None,
                 texture=math.fsum(q - x * x / m for q, x, m in zip(saa, sa, n)) / sum(n), roi_mse=s["roi_ssd"] / s["roi_pixels"])
        out.append(d)
    return out


GRATING_ROW_KEYS = ("gain", "thd", "response")   # what a grating_ row's "gratings" gathers, of the d profile
GRATING_ROW_STATS = ("median", "min", "max", "count")


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _grating_spread(summary):
    out = {"gratings": len(summary)}
    for k in GRATING_ROW_KEYS:
        v = [s[k] for s in summary if s[k] is not None]
        out[k] = {"median": _median(v), "min": min(v), "max": max(v), "count": len(v)} if v else {"median": None, "min": None, "max": None, "count": 0}
    return out


def grating_row(gratings, stats, sq_diff_sum, pixels, tables=False):
    """A grating_ row's "gratings" value from the row's gratings, their exact tables and the full frame's exact sum of squared
    differences over `pixels` pixels: {"all": spread, "directions": {"ux,uy": spread}, "periods": {T: spread}, in the order of first
    appearance and in ascending T, "outside_mse": (sq_diff_sum - sum roi_ssd) / (pixels - sum roi_pixels), the change away from every
    region}. A spread is {"gratings": the group's size, and for each of GRATING_ROW_KEYS its median, min and max over the gratings that
    have the number and their count}. With tables=True also "per_grating": the x, y, h, ux, uy, T, wave and grating_summary's dict of
    every grating, the folded profiles included, in the list's order."""
    summary = grating_summary(stats, gratings)
    out = {"all": _grating_spread(summary)}
    directions = list(dict.fromkeys((g[3], g[4]) for g in gratings))
    out["directions"] = {"%d,%d" % u: _grating_spread([s for g, s in zip(gratings, summary) if (g[3], g[4]) == u]) for u in directions}
    out["periods"] = {t: _grating_spread([s for g, s in zip(gratings, summary) if g[5] == t]) for t in sorted(set(g[5] for g in gratings))}
    rois, inside = sum(s["roi_ssd"] for s in stats), sum(s["roi_pixels"] for s in stats)
    outside = int(pixels) - inside
    out["outside_mse"] = (int(sq_diff_sum) - rois) / outside if outside else 0.0
    if tables:
        out["per_grating"] = [dict(s, x=g[0], y=g[1], h=g[2], ux=g[3], uy=g[4], T=g[5], wave=list(g[6])) for g, s in zip(gratings, summary)]
    return out


# ---- detector gain: the exact row and column profiles of a comparison (not in the reference's script) ---------------------------------
# Every other metric of the study reduces over areas: a defective column of 0.2 gray levels changes their numbers in the fifth digit.
# A profile integrates along the line, as the eye does, and shows it at once. profile_statistics is the contract of
# musica_sim_profiles (include/musica.h), which is bit-identical to it; profile_summary is what the study reports of the integers, one
# function for every path.

def profile_statistics(a, b, regions):
    """The exact column and row profiles of every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes: what
    musica_sim_profiles returns. One dict per region: "cols", a (w, 4) uint32 array, and "rows", (h, 4): per line the sums over the
    line's pixels inside the region of a, of b, of (a - b)^2 and of a^2 (processing.PROFILE_SUMS), h pixels for a column and w for a
    row; "ssd", the sum over the region of (a - b)^2, which both tables' third columns add up to; "pixels" = w h. A line of up to
    16364 pixels sums to less than 2^32."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("profile_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    out = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        pa, pb = a[ay:ay + h, ax:ax + w].astype(np.int64), b[by:by + h, bx:bx + w].astype(np.int64)
        sums = (pa, pb, (pa - pb) ** 2, pa * pa)
        out.append({"cols": np.stack([s.sum(axis=0) for s in sums], axis=1).astype(np.uint32),
                    "rows": np.stack([s.sum(axis=1) for s in sums], axis=1).astype(np.uint32), "ssd": int(sums[2].sum()), "pixels": w * h})
    return out


PROFILE_AXES = ("cols", "rows")     # a profile table's two axes: the lines are columns (gains gx), then rows (gains gy)
PROFILE_KEYS = ("mean_shift", "transfer", "corr", "residual_rms", "peak", "line_noise", "visibility", "spread")


def _profile_axis(table, n, gains):
    """profile_summary's dict of one axis: table (lines, 4) exact integers, n pixels per line, `gains` the lines' gains in 1 / GAIN_ONE."""
    lines = len(table)
    if len(gains) != lines:
        raise ValueError("a profile of %d lines needs %d gains, got %d" % (lines, lines, len(gains)))
    diff = [int(r[0]) - int(r[1]) for r in table]
    D = [d / n for d in diff]
    L = [int(g) / mp.GAIN_ONE - 1.0 for g in gains]
    mean_d, mean_l = math.fsum(D) / lines, math.fsum(L) / lines
    dc, lc = [d - mean_d for d in D], [v - mean_l for v in L]
    sdd, sll, sld = math.fsum(d * d for d in dc), math.fsum(v * v for v in lc), math.fsum(d * v for d, v in zip(dc, lc))
    flat = min(gains) == max(gains)             # decided on the integers: L is constant
    transfer = None if flat else sld / sll
    fit = [0.0 if flat else transfer * v for v in lc]
    peak = max(abs(d) for d in dc)
    # the pooled within-line sample variance of a - b, from exact integers: sum_i (n sum_dd_i - diff_i^2) / (n lines (n - 1))
    within = sum(n * int(r[2]) - d * d for r, d in zip(table, diff))
    noise = math.sqrt(within / (n * lines * (n - 1)) / n) if n > 1 else None
    ranked = sorted(int(g) for g in gains)
    median = ranked[lines // 2]
    return {"lines": lines, "mean_shift": mean_d, "transfer": transfer, "corr": sld / math.sqrt(sll * sdd) if not flat and sdd > 0.0 else None,
            "residual_rms": math.sqrt(math.fsum((d - f) ** 2 for d, f in zip(dc, fit)) / lines), "peak": peak, "line_noise": noise,
            "visibility": peak / noise if noise else None,
            "spread": math.fsum(d * d for d, g in zip(dc, gains) if int(g) == median) / sdd if sdd > 0.0 else None}


def profile_summary(tables, gx_out, gy_out):
    """What the study reports of a gain row, from profile_statistics' (or musica_sim_profiles') exact integers of ONE region and the gain
    tables of its columns and rows (in 1 / GAIN_ONE, w and h entries): one function for every study path and all five families, so the
    paths agree to the last bit. {"cols": d, "rows": d}; per axis, in f64, with n the pixels of a line (h for a column, w for a row),
        D[i] = (sum_a - sum_b) / n      the line's mean change, in gray levels (one correctly rounded division of two integers)
        L[i] = g[i] / GAIN_ONE - 1      the line's relative gain
    and Dc, Lc the two centred on their means (math.fsum):
        lines         how many
        mean_shift    the mean of D: what the whole frame moved by
        transfer      sum Lc Dc / sum Lc^2, the least-squares slope of D on L: gray levels per unit of relative gain; None where L is
                      constant (decided on the integer gains)
        corr          sum Lc Dc / sqrt(sum Lc^2 sum Dc^2); None where L or D is constant
        residual_rms  sqrt(mean (Dc - transfer Lc)^2): what the fit leaves (of Dc itself where transfer is None)
        peak          max |Dc|
        line_noise    the standard error of a line's mean: sqrt(s^2 / n) with the pooled within-line sample variance of a - b,
                      s^2 = sum_i (n sum_dd[i] - (sum_a[i] - sum_b[i])^2) / (n lines (n - 1)), the numerator an exact integer; None for n = 1
        visibility    peak / line_noise: how far the largest line stands out of what a line's mean scatters by; None where line_noise
                      is None or 0
        spread        the share of sum Dc^2 on the lines whose gain equals the axis's median gain (the upper median, an entry of the
                      table): how far a line or a step leaks into unaltered neighbours; 1 where every line has the median gain; None
                      where D is constant
    No threshold is fixed here: these are findings."""
    cols, rows = np.asarray(tables["cols"]), np.asarray(tables["rows"])
    return {"cols": _profile_axis(cols, len(rows), list(gx_out)), "rows": _profile_axis(rows, len(cols), list(gy_out))}


def profile_row(tables, gx_out, gy_out, keep=False):
    """A gain row's "profiles" value: profile_summary's dict, with keep=True also "tables": {"cols", "rows"} as lists of the lines'
    four integers and "gains": {"cols", "rows"} as lists."""
    out = profile_summary(tables, gx_out, gy_out)
    if keep:
        out["tables"] = {k: [[int(v) for v in r] for r in tables[k]] for k in PROFILE_AXES}
        out["gains"] = {"cols": [int(g) for g in gx_out], "rows": [int(g) for g in gy_out]}
    return out


# ---- tone tables: the output per level of the input (not in the reference's script) --------------------------------------------------
# Every other metric of the study compares the output with a reference plane; none conditions on the input. The sums of a comparison
# kept apart by the class of the INPUT pixel (its raw value >> shift) give the characteristic curve of the chain, the mean output per
# input level, before and after an alteration, and split the change into a part that is a function of the input level alone (a change
# of the global tone curve) and a remainder. level_statistics is the contract of musica_sim_levels (include/musica.h), which is
# bit-identical to it; level_summary is what the study reports of the integers, one function for every path.

def level_statistics(a, b, classes, regions, count):
    """The exact sums per class of every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes: what musica_sim_levels
    returns. `classes` is an integer plane of a's shape with values below `count` (1 .. 4096; harness.level_classes): the class of a
    pixel is taken at side a's coordinates, whatever origin side b has. One (count, 6) uint64 table per region: per class the sums over
    the region's pixels of that class of 1, a, b, (a - b)^2, a^2 and b^2 (processing.LEVEL_SUMS). The first column adds up to w h, the
    fourth to the region's sum of squared differences (musica_sim_compare's sq_diff_sum). Integers throughout: every sum is a
    histogram of (class, value) pairs times the values."""
    a, b, classes, count = np.asarray(a), np.asarray(b), np.asarray(classes), int(count)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("level_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    if not 1 <= count <= 4096:
        raise ValueError("count %d is not in 1 .. 4096" % count)
    if classes.shape != a.shape or classes.dtype.kind not in "iu" or (classes.size and (int(classes.min()) < 0 or int(classes.max()) >= count)):
        raise ValueError("the classes are not a %r plane of integers below %d, got %r %s" % (a.shape, count, classes.shape, classes.dtype))
    values, diffs = np.arange(256, dtype=np.int64), np.arange(-255, 256, dtype=np.int64)
    out = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        k = classes[ay:ay + h, ax:ax + w].astype(np.int64).ravel()
        pa, pb = a[ay:ay + h, ax:ax + w].astype(np.int64).ravel(), b[by:by + h, bx:bx + w].astype(np.int64).ravel()
        ha = np.bincount(k * 256 + pa, minlength=count * 256).reshape(count, 256)              # how often class k meets the value a
        hb = np.bincount(k * 256 + pb, minlength=count * 256).reshape(count, 256)
        hd = np.bincount(k * 511 + (pa - pb + 255), minlength=count * 511).reshape(count, 511)   # ... and the difference a - b
        out.append(np.stack([ha.sum(axis=1), ha @ values, hb @ values, hd @ (diffs * diffs), ha @ (values * values), hb @ (values * values)],
                            axis=1).astype(np.uint64))
    return out


LEVEL_KEYS = ("classes", "curve_shift_rms", "curve_shift_max", "slope", "correlation", "global_fraction", "within_rms", "spread_ratio", "reversals")


def level_summary(table, curves=False):
    """What the study reports of a lut row, from level_statistics' (or musica_sim_levels') exact integers of ONE region: one function
    for every study path, so the paths agree to the last bit. With k running over the OCCUPIED classes (n_k > 0) in ascending order,
    N = sum n_k, ssd = sum sum_dd, d_k = sum_a - sum_b (an integer), and in f64 (one correctly rounded division of two integers
    each, sums by math.fsum)
        a_k = sum_a / n_k, b_k = sum_b / n_k      the two characteristic curves: the mean output of class k after and before
    the dict holds
        classes          how many classes are occupied
        curve_shift_rms  sqrt(sum n_k (a_k - b_k)^2 / N), the terms taken as d_k^2 / n_k
        curve_shift_max  max |a_k - b_k|, taken as |d_k| / n_k
        slope            the n-weighted least-squares slope of a_k on b_k across the classes, sum n (a - ma)(b - mb) / sum n (b - mb)^2
                         with the n-weighted means ma, mb; None where b_k is constant
        correlation      sum n (a - ma)(b - mb) / sqrt(sum n (a - ma)^2 sum n (b - mb)^2); None where a_k or b_k is constant
        global_fraction  sum_k d_k^2 / n_k / ssd: the share of the change that is a function of the input level alone, hence a pure
                         change of the global tone curve; None where nothing changed (ssd = 0)
        within_rms       sqrt(sum_k (n_k sum_dd - d_k^2) / n_k / N), every numerator an exact non-negative integer: the within-class
                         remainder, so that global_fraction ssd + within_rms^2 N = ssd to rounding
        spread_ratio     sqrt(Wa / Wb) with W = sum_k (n_k sum_xx - sum_x^2) / n_k, the pooled within-class scatter of a over that of b:
                         whether local contrast at a given input level changed; None where Wb = 0
        reversals        how many neighbouring occupied classes have an a step and a b step of opposite non-zero signs, decided on the
                         integers (the sign of sum_x' n - sum_x n')
    and with curves=True also "levels" (the occupied classes), "curve_a" and "curve_b" (a_k and b_k) as lists. No threshold is fixed
    here: these are findings."""
    t = [[int(v) for v in row] for row in np.asarray(table)]
    if not t or any(len(row) != 6 for row in t):
        raise ValueError("a level table is (classes, 6), got %r" % (np.asarray(table).shape,))
    rows = [(k, row) for k, row in enumerate(t) if row[0] > 0]
    if not rows:
        raise ValueError("the level table holds no pixel")
    n = [r[0] for _, r in rows]
    total, ssd = sum(n), sum(r[3] for _, r in rows)
    d = [r[1] - r[2] for _, r in rows]
    a, b = [r[1] / r[0] for _, r in rows], [r[2] / r[0] for _, r in rows]
    between = math.fsum(v * v / m for v, m in zip(d, n))
    within = math.fsum((m * r[3] - v * v) / m for (_, r), v, m in zip(rows, d, n))
    ma, mb = sum(r[1] for _, r in rows) / total, sum(r[2] for _, r in rows) / total
    saa = math.fsum(m * (x - ma) ** 2 for m, x in zip(n, a))
    sbb = math.fsum(m * (y - mb) ** 2 for m, y in zip(n, b))
    sab = math.fsum(m * (x - ma) * (y - mb) for m, x, y in zip(n, a, b))
    flat_a, flat_b = (all(r[i] * n[0] == rows[0][1][i] * m for (_, r), m in zip(rows, n)) for i in (1, 2))   # decided on the integers
    wa = math.fsum((m * r[4] - r[1] * r[1]) / m for (_, r), m in zip(rows, n))
    wb = math.fsum((m * r[5] - r[2] * r[2]) / m for (_, r), m in zip(rows, n))
    reversals = 0
    for ((_, p), (_, q)) in zip(rows, rows[1:]):
        step_a, step_b = q[1] * p[0] - p[1] * q[0], q[2] * p[0] - p[2] * q[0]
        reversals += (step_a > 0 and step_b < 0) or (step_a < 0 and step_b > 0)
    out = {"classes": len(rows), "curve_shift_rms": math.sqrt(between / total), "curve_shift_max": max(abs(v) / m for v, m in zip(d, n)),
           "slope": None if flat_b else sab / sbb, "correlation": None if flat_a or flat_b else sab / math.sqrt(saa * sbb),
           "global_fraction": between / ssd if ssd else None, "within_rms": math.sqrt(within / total),
           "spread_ratio": math.sqrt(wa / wb) if wb > 0.0 else None, "reversals": int(reversals)}
    if curves:
        out.update(levels=[k for k, _ in rows], curve_a=a, curve_b=b)
    return out


def level_row(table, sq_diff_sum, pixels, keep=False):
    """A lut row's "levels" value: level_summary's dict of the full frame's table, with keep=True the two curves as well. The table
    must account for the frame (ValueError otherwise): its n add up to `pixels` and its sum_dd to `sq_diff_sum`, the integers of the
    row's direct comparison."""
    t = np.asarray(table)
    if int(t[:, 0].sum()) != int(pixels) or int(t[:, 3].sum()) != int(sq_diff_sum):
        raise ValueError("the level table holds %d pixels and a squared difference of %d, the frame %d and %d"
                         % (int(t[:, 0].sum()), int(t[:, 3].sum()), int(pixels), int(sq_diff_sum)))
    return level_summary(t, curves=keep)


# ---- gradient metrics: the edges of a comparison, by the edge strength of the reference (not in the reference's script) ---------------
# MUSICA raises weak gradients more than strong ones. Every other metric compares gray levels, windows, scales, positions, lines or
# planted patches; this one compares the integer Sobel gradients of both sides of a comparison over the interior of its region, their
# exact sums kept apart by the bit length of the reference side's squared gradient. gradient_statistics is the contract of
# musica_sim_gradients (include/musica.h), whose tables are bit-identical to it; gradient_summary is what the study reports of the
# integers, one function for every path.

def sobel_gradients(p):
    """The integer Sobel gradients (gx, gy), int64, of a 2-D plane over its interior, (h - 2, w - 2):
    gx = (p[y-1][x+1] + 2 p[y][x+1] + p[y+1][x+1]) - (the same at x - 1), gy = (p[y+1][x-1] + 2 p[y+1][x] + p[y+1][x+1]) - (the same
    at y - 1); for a uint8 plane both lie in -1020 .. 1020."""
    p = np.asarray(p).astype(np.int64)
    col = p[:-2, :] + 2 * p[1:-1, :] + p[2:, :]     # t + 2 m + b of every column
    row = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    return col[:, 2:] - col[:, :-2], row[2:, :] - row[:-2, :]


def gradient_statistics(out, ref, regions):
    """What musica_sim_gradients returns for every region (ax, ay, bx, by, w, h), w, h >= 7, of two 2-D uint8 planes (side a: `out`,
    side b: `ref`): a list of (table, gsim). Over the interior of the region, the (w - 2) x (h - 2) pixels whose 3 x 3 neighbourhood
    lies inside it, with the gradients of sobel_gradients and per pixel
        A = gxa^2 + gya^2, B = gxb^2 + gyb^2, dot = gxa gxb + gya gyb, cross = gxa gyb - gya gxb      (each |.| <= 1 300 500)
    a pixel's class is the bit length of B, 0 .. 21 (processing.GRADIENT_CLASSES = 22): 0 where the reference has no gradient. The
    table is (22, 6) uint64, per class n, sum A, sum B, sum dot, sum cross (both signed, stored in two's complement as the device
    stores them: table.view(np.int64) reads them) and neg, the number of its pixels with dot < 0 (processing.GRADIENT_FIELDS); exact
    integers, the n adding up to (w - 2)(h - 2). gsim is the mean over the interior of q = (2 dot + C) / (A + B + C), C =
    processing.GRADIENT_C = 2720 (the 170 of GMSD, Xue et al. 2014, for Prewitt / 3, carried to Sobel's squared scale: x 16): one
    correctly rounded f64 division of two exact integers per pixel, summed by math.fsum; identical sides give exactly 1.0."""
    a, b = np.asarray(out), np.asarray(ref)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("gradient_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 7 or h < 7 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is smaller than 7 x 7 or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        gxa, gya = sobel_gradients(a[ay:ay + h, ax:ax + w])
        gxb, gyb = sobel_gradients(b[by:by + h, bx:bx + w])
        A, B = gxa * gxa + gya * gya, gxb * gxb + gyb * gyb
        dot, cross = gxa * gxb + gya * gyb, gxa * gyb - gya * gxb
        cls = np.frexp(B.astype(np.float64))[1]      # the bit length of an integer below 2^53: frexp's exponent, 0 for 0
        table = np.zeros((mp.GRADIENT_CLASSES, len(mp.GRADIENT_FIELDS)), dtype=np.int64)
        for k in np.unique(cls):
            m = cls == k
            table[k] = [int(m.sum()), int(A[m].sum()), int(B[m].sum()), int(dot[m].sum()), int(cross[m].sum()), int((dot[m] < 0).sum())]
        q = (2 * dot + mp.GRADIENT_C).astype(np.float64) / (A + B + mp.GRADIENT_C).astype(np.float64)
        res.append((table.view(np.uint64), math.fsum(q.ravel().tolist()) / q.size))
    return res


GRADIENT_KEYS = ("gsim", "gc", "gain", "turn", "reversed", "rmse", "compression")   # gradient_summary's numbers, before gain_by_class


def _signed_table(table):
    t = np.asarray(table)
    if t.shape != (mp.GRADIENT_CLASSES, len(mp.GRADIENT_FIELDS)) or t.dtype.kind not in "iu":
        raise ValueError("a gradient table is (%d, %d) integers, got %r %s" % (mp.GRADIENT_CLASSES, len(mp.GRADIENT_FIELDS), t.shape, t.dtype))
    t = t.astype(np.uint64).view(np.int64) if t.dtype.kind == "u" else t
    return [[int(v) for v in row] for row in t]


def gradient_summary(table, gsim):
    """What the study reports of a comparison's gradients, from gradient_statistics' (or musica_sim_gradients') exact integers of ONE
    region: one function for every study path. With the sums over all classes N, SA, SB, SD (dot), SC (cross), exact integers:
        gsim           as given
        gc             SD / sqrt(SA SB), the gradient correlation; 1.0 where both sides are flat (SA = SB = 0), 0.0 where one is
        gain           sqrt(SA / SB); 1.0 where both sides are flat, None where only the reference is (SB = 0 < SA)
        turn           atan2(SC, SD) in degrees, the mean rotation of the gradients from b to a; 0.0 where SC = SD = 0
        reversed       the share of the pixels of classes >= 1 with dot < 0; 0.0 where there is none (a flat reference)
        rmse           sqrt((SA + SB - 2 SD) / N), the rms length of the gradient difference (the numerator is sum |ga - gb|^2 >= 0)
        gain_by_class  22 entries, sqrt(sum A / sum B) of the class; None where the class is empty or its sum B is 0 (class 0)
        compression    the n-weighted least-squares slope of log2(gain_by_class) on the class index over the classes >= 1 that have a
                       positive gain; 0.0 with fewer than two such classes. Negative where weak edges are amplified more than strong
                       ones, MUSICA's signature.
    Every float is one correctly rounded operation on exact integers, or math.fsum of such. ValueError for a table without a pixel."""
    t = _signed_table(table)
    n, sa, sb, sd, sc = (sum(row[i] for row in t) for i in range(5))
    if n <= 0:
        raise ValueError("the gradient table holds no pixel")
    edged, neg = sum(row[0] for row in t[1:]), sum(row[5] for row in t[1:])
    gains = [math.sqrt(row[1] / row[2]) if row[0] > 0 and row[2] > 0 else None for row in t]
    fit = [(k, t[k][0], math.log2(g)) for k, g in enumerate(gains) if k >= 1 and g is not None and g > 0.0]
    compression = 0.0
    if len(fit) >= 2:
        weight = sum(m for _, m, _ in fit)
        mk, my = sum(m * k for k, m, _ in fit) / weight, math.fsum(m * y for _, m, y in fit) / weight
        compression = math.fsum(m * (k - mk) * (y - my) for k, m, y in fit) / math.fsum(m * (k - mk) ** 2 for k, m, _ in fit)
    return {"gsim": float(gsim),
            "gc": sd / math.sqrt(sa * sb) if sa and sb else 1.0 if sa == sb else 0.0,
            "gain": math.sqrt(sa / sb) if sb else 1.0 if sa == 0 else None,
            "turn": math.degrees(math.atan2(sc, sd)),
            "reversed": neg / edged if edged else 0.0,
            "rmse": math.sqrt((sa + sb - 2 * sd) / n),
            "compression": compression,
            "gain_by_class": gains}


def gradient_row(table, gsim):
    """A row's *_gradient value: gradient_summary's dict and "table", the 22 x 6 exact integers (dot and cross signed) as lists."""
    return dict(gradient_summary(table, gsim), table=_signed_table(table))


# ---- local order: the census signs of a comparison (not in the reference's script) -----------------------------------------------------
# MUSICA ends in a monotone tone curve and most alterations move gray levels without changing the scene. Every other metric charges the
# values that moved; this one asks whether the same pixel is still the darker one of a neighbouring pair (the census transform, Zabih &
# Woodfill 1994): a spatially varying but locally monotone change keeps every local order and scores as "nothing happened", while
# rebound rings, halos, reversed weak edges and flattened texture break orders. order_statistics is the contract of musica_sim_order
# (include/musica.h), whose tables are bit-identical to it; order_summary is what the study reports of the integers, one function for
# every path. Integers throughout: every double is computed here from exact integers.

ORDER_RADIUS = 3   # the 7 x 7 neighbourhood: rings max(|dx|, |dy|) = 1, 2, 3 with 8, 16 and 24 neighbours


def order_statistics(out, ref, regions):
    """What musica_sim_order returns for every region (ax, ay, bx, by, w, h), w, h >= 7, of two 2-D uint8 planes (side a: `out`, side
    b: `ref`): a list of flat tables of processing.ORDER_TABLE_WORDS = 112 uint64. Over the interior of the region, the (w - 6) x
    (h - 6) pixels whose 7 x 7 neighbourhood lies inside it, a pixel c and each of its 48 neighbours n give per side the sign
    s = sign(p[n] - p[c]); the pair is `same` (sa = sb != 0), `reversed` (sa = -sb != 0), `flattened` (sa = 0, sb != 0: the output ties
    where the reference orders), `split` (sa != 0, sb = 0) or tied on both sides. The table holds first (3, 5), per ring max(|dx|, |dy|)
    = 1, 2, 3 the pairs (pixels x 8, 16, 24), same, reversed, flattened and split (processing.ORDER_FIELDS), then the (97,) histogram
    of the per-pixel census distance d = sum |sa - sb| = 2 reversed + flattened + split, 0 .. 96 (order_parts splits a table)."""
    a, b = np.asarray(out), np.asarray(ref)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("order_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    R = ORDER_RADIUS
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 7 or h < 7 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is smaller than 7 x 7 or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        pa, pb = a[ay:ay + h, ax:ax + w].astype(np.int16), b[by:by + h, bx:bx + w].astype(np.int16)
        ca, cb = pa[R:h - R, R:w - R], pb[R:h - R, R:w - R]
        rings = np.zeros((mp.ORDER_RINGS, len(mp.ORDER_FIELDS)), dtype=np.int64)
        d = np.zeros(ca.shape, dtype=np.int64)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ring = max(abs(dx), abs(dy))
                if ring == 0:
                    continue
                sa = np.sign(pa[R + dy:h - R + dy, R + dx:w - R + dx] - ca)
                sb = np.sign(pb[R + dy:h - R + dy, R + dx:w - R + dx] - cb)
                rings[ring - 1] += [ca.size, int(((sa == sb) & (sa != 0)).sum()), int(((sa == -sb) & (sa != 0)).sum()),
                                    int(((sa == 0) & (sb != 0)).sum()), int(((sa != 0) & (sb == 0)).sum())]
                d += np.abs(sa - sb)
        res.append(np.concatenate([rings.ravel(), np.bincount(d.ravel(), minlength=mp.ORDER_BINS)]).astype(np.uint64))
    return res


ORDER_KEYS = ("tau", "tau_by_ring", "reversed", "flattened", "split", "intact", "distance", "median", "p95")   # order_summary's numbers


def order_parts(table):
    """A flat order table as (rings, histogram): lists of Python ints, 3 x 5 and 97. ValueError for anything but 112 integers."""
    t = np.asarray(table)
    if t.shape != (mp.ORDER_TABLE_WORDS,) or t.dtype.kind not in "iu":
        raise ValueError("an order table is %d integers, got %r %s" % (mp.ORDER_TABLE_WORDS, t.shape, t.dtype))
    v = [int(x) for x in t]
    head = mp.ORDER_RINGS * len(mp.ORDER_FIELDS)
    return [v[r * len(mp.ORDER_FIELDS):(r + 1) * len(mp.ORDER_FIELDS)] for r in range(mp.ORDER_RINGS)], v[head:]


def _order_tau(same, rev, flat, split):
    strict_a, strict_b = same + rev + split, same + rev + flat
    if strict_a == 0 or strict_b == 0:
        return 1.0 if strict_a == strict_b else 0.0
    return (same - rev) / math.sqrt(strict_a * strict_b)


def _order_rank(hist, num, den):
    """The smallest d whose cumulative count reaches num / den of the pixels (nearest rank, integers only)."""
    total, cum = sum(hist), 0
    for d, n in enumerate(hist):
        cum += n
        if n and cum * den >= total * num:
            return d
    return 0


def order_summary(table):
    """What the study reports of a comparison's local order, from order_statistics' (or musica_sim_order's) exact integers of ONE
    region: one function for every study path. With the sums over the rings N (pairs), S (same), R (reversed), F (flattened), P (split):
        tau          (S - R) / sqrt((S + R + P)(S + R + F)): Kendall's tau-b restricted to centre-neighbour pairs (the factors are the
                     pairs strict in a and strict in b); 1.0 where both sides tie everywhere, 0.0 where exactly one does
        tau_by_ring  the same of each ring alone, three entries
        reversed     R / (S + R), the share of the pairs ordered on both sides whose order is reversed; 0.0 without such a pair
        flattened    F / (S + R + F), the share of the pairs strict in b that a ties; 0.0 where b ties everywhere
        split        P / (N - (S + R + F)), the share of the pairs tied in b that a orders; 0.0 where b ties nowhere
        intact       hist[0] / pixels, the share of the pixels whose 48 signs all agree
        distance     the mean census distance / 96
        median, p95  of d, nearest rank: the smallest d whose cumulative count reaches 1 / 2 and 95 / 100 of the pixels (ints)
    Every float is one or two correctly rounded operations on exact integers. ValueError for a table without a pixel, or whose
    histogram and rings disagree (sum hist = pairs / 8, 16, 24; sum d hist[d] = sum 2 R + F + P)."""
    rings, hist = order_parts(table)
    pixels = sum(hist)
    n, s, r, f, p = (sum(row[i] for row in rings) for i in range(5))
    if pixels <= 0:
        raise ValueError("the order table holds no pixel")
    if [row[0] for row in rings] != [pixels * 8 * (k + 1) for k in range(mp.ORDER_RINGS)] or sum(d * v for d, v in enumerate(hist)) != 2 * r + f + p:
        raise ValueError("the order table's histogram holds %d pixels at a distance sum of %d, its rings %r pairs and %d"
                         % (pixels, sum(d * v for d, v in enumerate(hist)), [row[0] for row in rings], 2 * r + f + p))
    strict_b = s + r + f
    return {"tau": _order_tau(s, r, f, p),
            "tau_by_ring": [_order_tau(*row[1:]) for row in rings],
            "reversed": r / (s + r) if s + r else 0.0,
            "flattened": f / strict_b if strict_b else 0.0,
            "split": p / (n - strict_b) if n - strict_b else 0.0,
            "intact": hist[0] / pixels,
            "distance": (2 * r + f + p) / (96 * pixels),
            "median": _order_rank(hist, 1, 2),
            "p95": _order_rank(hist, 95, 100)}


def order_row(table):
    """A row's *_order value: order_summary's dict, "rings", the 3 x 5 exact integers, and "histogram", the 97, as lists."""
    rings, hist = order_parts(table)
    return dict(order_summary(table), rings=rings, histogram=hist)


# ---- reach: the change of the output by the distance from the changed input (not in the reference's script) ---------------------------
# The locality relation: a change of the input inside a set changes the output only near it. Two effects carry a local change outwards:
# the pyramid's footprints (a level-i band reaches about 2^(i + 2) pixels and dies off with distance) and the global stages (min / max,
# the histograms, the tone curve: the same small shift everywhere). The sums of a comparison kept apart by the Chebyshev distance of the
# pixel from the nearest changed input pixel tell them apart. reach_classes and reach_statistics are the contract of musica_sim_reach
# and musica_sim_reach_classes (include/musica.h), which are bit-identical to them; reach_summary is what the study reports of the
# integers, one function for every path.

def reach_classes(source, altered, radii):
    """The reach class of every pixel of two 2-D uint16 planes of one shape, a uint8 plane: with seed = source != altered and the K radii
    (processing.reach_radii: radii[0] = 0, strictly ascending, at most 32 of at most 16383), the class of pixel (x, y) is the smallest k
    for which the box [x - radii[k], x + radii[k]] x [y - radii[k], y + radii[k]], clipped to the plane, holds a seed, and K where the
    box of radii[K - 1] holds none (also where nothing changed at all). Class 0 is a changed pixel itself. A box of radius r holds a seed
    exactly where the Chebyshev distance to the nearest seed is at most r, so this is the chessboard distance transform of the seeds
    (scipy.ndimage.distance_transform_cdt), looked up in the radii: no summed-area table, unlike the device."""
    s, a = np.asarray(source), np.asarray(altered)
    if s.ndim != 2 or s.shape != a.shape or s.dtype != np.uint16 or a.dtype != np.uint16:
        raise ValueError("reach_classes needs two 2-D uint16 planes of one shape, got %r %s and %r %s" % (s.shape, s.dtype, a.shape, a.dtype))
    r = mp.reach_radii(radii)
    seed = s != a
    if not seed.any():
        return np.full(s.shape, len(r), dtype=np.uint8)
    dist = ndimage.distance_transform_cdt(~seed, metric="chessboard")    # 0 on a seed, else the L-infinity distance to the nearest one
    return np.searchsorted(r.astype(np.int64), dist.astype(np.int64), side="left").astype(np.uint8)


def reach_statistics(out, ref, classes, regions, count):
    """The exact sums per reach class of every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a: `out`, side b:
    `ref`): what musica_sim_reach returns. `classes` is reach_classes' plane of the INPUT, 2 * OUT_MARGIN larger than `out` along both
    axes, with values below `count` = K + 1: the class of a-side pixel (x, y) is classes[y + OUT_MARGIN, x + OUT_MARGIN], whatever
    origin side b has. One (count, 6) uint64 table per region: per class n, changed (the pixels with a != b), sum_a, sum_b, sum_dd = the
    sum of (a - b)^2 and max_d = max |a - b|, 0 for an empty class (processing.REACH_FIELDS). The n add up to w h, the sum_dd to the
    region's sum of squared differences (musica_sim_compare's sq_diff_sum); changed <= n and max_d^2 changed >= sum_dd >= changed."""
    a, b, classes, count = np.asarray(out), np.asarray(ref), np.asarray(classes), int(count)
    m = mp.OUT_MARGIN
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("reach_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    if not 2 <= count <= mp.REACH_MAX_RADII + 1:
        raise ValueError("count %d is not in 2 .. %d" % (count, mp.REACH_MAX_RADII + 1))
    if classes.shape != (a.shape[0] + 2 * m, a.shape[1] + 2 * m) or classes.dtype.kind not in "iu" or int(classes.min()) < 0 or int(classes.max()) >= count:
        raise ValueError("the classes are not a %r plane of integers below %d, got %r %s" % ((a.shape[0] + 2 * m, a.shape[1] + 2 * m), count, classes.shape, classes.dtype))
    values, tables = np.arange(256, dtype=np.int64), []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        k = classes[ay + m:ay + m + h, ax + m:ax + m + w].astype(np.int64).ravel()
        pa, pb = a[ay:ay + h, ax:ax + w].astype(np.int64).ravel(), b[by:by + h, bx:bx + w].astype(np.int64).ravel()
        ha = np.bincount(k * 256 + pa, minlength=count * 256).reshape(count, 256)                # how often class k meets the value a
        hb = np.bincount(k * 256 + pb, minlength=count * 256).reshape(count, 256)
        hd = np.bincount(k * 256 + np.abs(pa - pb), minlength=count * 256).reshape(count, 256)   # ... and the difference |a - b|
        n = hd.sum(axis=1)
        max_d = np.where(hd > 0, values, 0).max(axis=1)
        tables.append(np.stack([n, n - hd[:, 0], ha @ values, hb @ values, hd @ (values * values), max_d], axis=1).astype(np.uint64))
    return tables


REACH_KEYS = ("seeds", "classes", "last_class", "extent", "floor", "spill", "half_reach", "decay")   # reach_summary's numbers over the table


def reach_summary(table, radii):
    """What the study reports of a comparison's reach, from reach_statistics' (or musica_sim_reach's) exact integers of ONE region: one
    function for every study path, so the paths agree to the last bit. The table has K + 1 rows for the K radii; class 0 is distance 0,
    class k in 1 .. K - 1 the distances radii[k - 1] + 1 .. radii[k], class K everything beyond radii[K - 1]. Every float is one
    correctly rounded operation on exact integers, or math.fsum of such in ascending class order. Per class, as lists of K + 1 entries
    (None where the class is empty, n = 0):
        n             the class's pixels (0 for an empty class)
        rmse          sqrt(sum_dd / n)
        changed       changed / n, the share of its pixels whose output changed
        shift         (sum_a - sum_b) / n, the mean signed change
        max           max_d
        outer         radii[k], the class's outer radius; None for the open class K
    and over the table
        classes       how many classes are occupied
        last_class    the largest class with changed > 0; None where no pixel changed
        extent        the outer radius of last_class: beyond it NOTHING changed, exactly; None where last_class is None or the open
                      class K (the change reaches past the last radius)
        floor         the rmse of the outermost occupied class: the global component, which no distance removes
        spill         sum of sum_dd over the classes >= 1 / sum over all: the share of the change that left the altered set; None where
                      nothing changed (sum_dd = 0 everywhere)
        half_reach    the radius within which half of the spill lies. With T = the spill's sum_dd, C_k = sum_dd of classes 1 .. k
                      (C_0 = 0) and k the smallest class >= 1 with 2 C_k >= T (decided on the integers): linear in the radius across
                      class k, radii[k - 1] + (radii[k] - radii[k - 1]) (T - 2 C_{k-1}) / (2 sum_dd_k); None where T = 0 or k is the
                      open class K
        decay         the unweighted least-squares slope of log2(rmse_k^2 - floor^2) on log2(mid_k), mid_k = (radii[k - 1] + 1 +
                      radii[k]) / 2 the class's mean distance, over the occupied classes k in 1 .. K - 1 whose rmse^2 exceeds floor^2
                      (decided on the integers: sum_dd_k n_f > sum_dd_f n_k, f the floor's class; the difference is taken as
                      (sum_dd_k n_f - sum_dd_f n_k) / (n_k n_f)); None with fewer than three such classes. -2 is a 1 / r fall of the
                      amplitude.
    No threshold is fixed here: these are findings."""
    r = [int(v) for v in mp.reach_radii(radii)]
    t = [[int(v) for v in row] for row in np.asarray(table)]
    K = len(r)
    if len(t) != K + 1 or any(len(row) != 6 for row in t):
        raise ValueError("a reach table of %d radii is (%d, 6), got %r" % (K, K + 1, np.asarray(table).shape))
    occupied = [k for k in range(K + 1) if t[k][0] > 0]
    if not occupied:
        raise ValueError("the reach table holds no pixel")
    per = lambda f: [f(t[k]) if t[k][0] > 0 else None for k in range(K + 1)]
    touched = [k for k in occupied if t[k][1] > 0]
    last = touched[-1] if touched else None
    f = occupied[-1]
    nf, df = t[f][0], t[f][4]
    total, spilled = sum(row[4] for row in t), sum(row[4] for row in t[1:])
    half = None
    if spilled > 0:
        before = 0
        for k in range(1, K + 1):
            if 2 * (before + t[k][4]) >= spilled:
                if k < K:
                    half = r[k - 1] + (r[k] - r[k - 1]) * ((spilled - 2 * before) / (2 * t[k][4]))
                break
            before += t[k][4]
    fit = [(math.log2((r[k - 1] + 1 + r[k]) / 2), math.log2((t[k][4] * nf - df * t[k][0]) / (t[k][0] * nf)))
           for k in occupied if 1 <= k < K and t[k][4] * nf > df * t[k][0]]
    decay = None
    if len(fit) >= 3:
        mx, my = math.fsum(x for x, _ in fit) / len(fit), math.fsum(y for _, y in fit) / len(fit)
        decay = math.fsum((x - mx) * (y - my) for x, y in fit) / math.fsum((x - mx) ** 2 for x, _ in fit)
    return {"classes": len(occupied), "last_class": last, "extent": r[last] if last is not None and last < K else None,
            "floor": math.sqrt(df / nf), "spill": spilled / total if total else None, "half_reach": half, "decay": decay,
            "n": [row[0] for row in t], "rmse": per(lambda row: math.sqrt(row[4] / row[0])), "changed": per(lambda row: row[1] / row[0]),
            "shift": per(lambda row: (row[2] - row[3]) / row[0]), "max": per(lambda row: row[5]), "outer": r + [None]}


def reach_maps(class_plane, rmse):
    """Two uint8 images of a row's reach: the class plane, class 0 white and the last class black in equal steps, and the per-class rmse
    as bars, 8 pixels wide and up to 64 high, the tallest the largest rmse (an empty class and an rmse of 0 have no bar)."""
    plane = np.asarray(class_plane)
    last = len(rmse) - 1
    shade = (255 - (plane.astype(np.int64) * 255) // max(last, 1)).astype(np.uint8)
    top = max([v for v in rmse if v] or [1.0])
    bars = np.zeros((64, 8 * len(rmse)), np.uint8)
    for k, v in enumerate(rmse):
        h = int(round(64 * v / top)) if v else 0
        if h:
            bars[64 - h:, 8 * k:8 * k + 7] = 255
    return shade, bars


def reach_row(table, radii, seeds, sq_diff_sum, pixels, keep=False):
    """A row's direct_reach value: reach_summary's dict of the full frame's table, "seeds" (the changed pixels of the input plane) and
    "radii", with keep=True "table" as well, the (K + 1) x 6 exact integers as lists. The table must account for the frame (ValueError
    otherwise): its n add up to `pixels` and its sum_dd to `sq_diff_sum`, the integers of the row's direct comparison."""
    t = np.asarray(table)
    if int(t[:, 0].sum()) != int(pixels) or int(t[:, 4].sum()) != int(sq_diff_sum):
        raise ValueError("the reach table holds %d pixels and a squared difference of %d, the frame %d and %d"
                         % (int(t[:, 0].sum()), int(t[:, 4].sum()), int(pixels), int(sq_diff_sum)))
    out = dict(reach_summary(t, radii), seeds=int(seeds), radii=[int(v) for v in radii])
    if keep:
        out["table"] = [[int(v) for v in row] for row in t]
    return out


# ---- model observer: the channel responses of patches (not in the reference's script) ---------------------------------------------------
# Task-based assessment puts a model observer on top of MTF, noise power and contrast-detail: it looks at a patch through a few smooth
# channels and reports how well a disc is told from its absence against the background the processor produced, a detectability d'.
# detail_summary's cnr and rose are a one-number observer: they see neither the shape of the response (a halo or rebound ring) nor the
# correlation of the background. A channelized Hotelling observer with Laguerre-Gauss channels (Barrett & Myers, Foundations of Image
# Science, ch. 14; Gallas & Barrett 2003) is the standard answer. A view is (x, y, bank): an integer centre and the index of a bank, an
# int8 array (C, S, S) of C templates over the window |dx|, |dy| <= half, S = 2 half + 1; windows may overlap and views may repeat
# (processing.view_list). channel_responses is integer and the contract of musica_sim_observer (include/musica.h), which is
# bit-identical to it; observer_summary is the one f64 function every study path shares.

def channel_responses(a, b, views, banks):
    """The responses of every view of `views` (processing.view_list for the planes' side, else ValueError before any work) over two
    square uint8 planes of equal shape: a list of dicts, "a" and "b" the int32 arrays of the bank's C inner products
        R[j] = sum over dy, dx of bank[j, dy + half, dx + half] * plane[y + dy, x + dx]
    on either side (|R| <= 255 * 128 * 133^2 < 2^31; summed in int64), and the Python ints "pixels" = S^2, "sum_a" and "sum_b", the
    window's plain sums: what musica_sim_observer returns."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or a.shape != b.shape or a.shape[0] != a.shape[1] or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("channel_responses needs two square 2-D uint8 planes of equal shape, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    views, banks = mp.view_list(views, banks, a.shape[0])
    wide = [k.astype(np.int64) for k in banks]
    out = []
    for x, y, k in views:
        half = banks[k].shape[1] // 2
        pa = a[y - half:y + half + 1, x - half:x + half + 1].astype(np.int64)
        pb = b[y - half:y + half + 1, x - half:x + half + 1].astype(np.int64)
        out.append({"a": (wide[k] * pa[None]).sum(axis=(1, 2)).astype(np.int32), "b": (wide[k] * pb[None]).sum(axis=(1, 2)).astype(np.int32),
                    "pixels": int(pa.size), "sum_a": int(pa.sum()), "sum_b": int(pb.sum())})
    return out


OBSERVER_CHANNELS = 6   # the Laguerre-Gauss channels of the study's banks; the disc indicator follows them


def laguerre_gauss_bank(r, channels=OBSERVER_CHANNELS):
    """The study's bank for a radius-r detail: an int8 array (channels + 1, S, S) over the detail's box, half = 2r + 2, S = 2 half + 1.
    With rho2 = dx^2 + dy^2 and the width a = half, channel j < channels is the Laguerre-Gauss function
        u_j = exp(-pi rho2 / a^2) L_j(2 pi rho2 / a^2)                      (numpy.polynomial.laguerre)
    quantised as rint(127 u_j / max |u_j|): rotationally symmetric, so invariant under the square's eight symmetries, channel 0 a
    Gaussian with 127 at the centre (its only 127 up to r = 8; from r = 16 on the nearest neighbours round to 127 as well). The last
    channel is the disc indicator rho2 <= r^2 with weight 1: its response is detail_statistics' disc sum_a / sum_b, a cross-check
    between two entry points, and the non-prewhitening observer's template."""
    r, channels = int(r), int(channels)
    if r < 1 or not 1 <= channels < mp.OBSERVER_MAX_CHANNELS:
        raise ValueError("laguerre_gauss_bank needs r >= 1 and 1 .. %d channels, got r = %d and %d" % (mp.OBSERVER_MAX_CHANNELS - 1, r, channels))
    half = 2 * r + 2
    d = np.arange(-half, half + 1, dtype=np.int64)
    rho2 = d[:, None] ** 2 + d[None, :] ** 2
    t = np.pi * rho2.astype(np.float64) / float(half * half)
    bank = np.empty((channels + 1,) + rho2.shape, dtype=np.int8)
    for j in range(channels):
        u = np.exp(-t) * np.polynomial.laguerre.lagval(2.0 * t, [0.0] * j + [1.0])
        bank[j] = np.rint(127.0 * u / np.abs(u).max()).astype(np.int8)
    bank[channels] = rho2 <= r * r
    return bank


_OBSERVER_BANKS = {}


def observer_views(details):
    """(views, banks) of a detail list for channel_responses / sim_observer: one view per detail, in the list's order, at the detail's
    centre with the bank of its radius; the banks laguerre_gauss_bank(r) of the distinct radii in ascending order (each built once)."""
    radii = sorted(set(int(d[2]) for d in details))
    for r in radii:
        if r not in _OBSERVER_BANKS:
            _OBSERVER_BANKS[r] = laguerre_gauss_bank(r)
    return [(int(d[0]), int(d[1]), radii.index(int(d[2]))) for d in details], [_OBSERVER_BANKS[r] for r in radii]


OBSERVER_KEYS = ("count", "cho", "auc", "npw", "spread", "channel_snr")   # observer_summary's entries of one radius
OBSERVER_MAX_COND = 1e10                                                  # a covariance worse conditioned than this is not inverted


def _quotient(num, den):
    return num / den if den else None


def observer_summary(radii, responses):
    """What the study reports of the views of a cd_ row, from channel_responses' (or musica_sim_observer's) exact integers: one function
    for every study path, so the paths agree to the last bit. radii: the radius of each view's detail; responses: their dicts, the
    last channel of each the disc indicator, the others the LG channels. Per radius, over its m positions, with va_i and vb_i the LG
    responses on either side and D_i = va_i - vb_i, in f64:
        mean D      the mean signal in channel space
        K           (cov(va) + cov(vb)) / 2 with ddof = 1: the background's channel covariance
        cho         sqrt(max(mean D^T K^-1 mean D, 0)) by np.linalg.solve: the channelized Hotelling observer's detectability d'
        auc         (1 + erf(cho / 2)) / 2: the area under its ROC curve
        channel_snr mean D_j / sqrt(K_jj) per LG channel
        npw         the same quotient on the disc channel: the non-prewhitening observer with the disc as its template
        spread      std / |mean| (population std) of the Hotelling scores (K^-1 mean D)^T D_i over the positions: position invariance
    cho, auc and spread are None where m < 2 channels + 2 or cond(K) > OBSERVER_MAX_COND (a singular K among them); a quotient with a
    zero denominator is None, and with m < 2 there is no covariance at all. Returns {r: dict of OBSERVER_KEYS} in ascending r. No
    threshold is fixed here: these are findings."""
    out = {}
    for r in sorted(set(int(v) for v in radii)):
        group = [s for v, s in zip(radii, responses) if int(v) == r]
        va = np.array([[int(x) for x in s["a"]] for s in group], dtype=np.float64)
        vb = np.array([[int(x) for x in s["b"]] for s in group], dtype=np.float64)
        m, channels = va.shape[0], va.shape[1] - 1
        delta = va - vb
        mean = delta.mean(axis=0)
        entry = {"count": m, "cho": None, "auc": None, "npw": None, "spread": None, "channel_snr": [None] * channels}
        out[r] = entry
        if m < 2:
            continue
        full = 0.5 * (np.cov(va, rowvar=False, ddof=1) + np.cov(vb, rowvar=False, ddof=1)).reshape(channels + 1, channels + 1)
        snr = [_quotient(float(mean[j]), math.sqrt(max(float(full[j, j]), 0.0))) for j in range(channels + 1)]
        entry["channel_snr"], entry["npw"] = snr[:channels], snr[channels]
        k = full[:channels, :channels]
        if m < 2 * channels + 2 or not np.all(np.isfinite(k)) or not np.linalg.cond(k) <= OBSERVER_MAX_COND:
            continue
        w = np.linalg.solve(k, mean[:channels])
        cho = math.sqrt(max(float(mean[:channels] @ w), 0.0))
        scores = delta[:, :channels] @ w
        entry["cho"], entry["auc"] = cho, 0.5 * (1.0 + math.erf(cho / 2.0))
        entry["spread"] = _quotient(float(scores.std()), abs(float(scores.mean())))
    return out


def observer_row(details, responses):
    """A cd_ row's "observer" value from the row's details (their radii) and the responses of observer_views' views:
    {"radii": observer_summary's dict}."""
    return {"radii": observer_summary([d[2] for d in details], responses)}


def observer_curve(rows, level=1.0):
    """The contrast-detail curve of a study by its model observer: {r: the contrast (in 1 / 1024, a float) at which the cd_ rows' cho of
    radius r crosses `level`}, by linear interpolation in log-log between the first two neighbouring contrasts (ascending) whose cho lie
    on either side of it; None where it never crosses (a cho that is None or not positive is left out). The level is the caller's
    convention, not a finding."""
    if not level > 0:
        raise ValueError("observer_curve needs a positive level, got %r" % (level,))
    points = {}
    for row in rows:
        if row["alteration"].startswith("cd_") and row.get("observer"):
            for r, entry in row["observer"]["radii"].items():
                if entry["cho"] is not None and entry["cho"] > 0:
                    points.setdefault(r, []).append((int(row["alteration"][3:]), entry["cho"]))
    curve = {}
    for r in sorted(points):
        curve[r] = None
        pts = sorted(points[r])
        for (c1, h1), (c2, h2) in zip(pts, pts[1:]):
            if h1 == level:
                curve[r] = float(c1)
            elif h2 == level:
                curve[r] = float(c2)
            elif (h1 < level) != (h2 < level):
                t = (math.log(level) - math.log(h1)) / (math.log(h2) - math.log(h1))
                curve[r] = math.exp(math.log(c1) + t * (math.log(c2) - math.log(c1)))
            else:
                continue
            break
        if curve[r] is None and len(pts) == 1 and pts[0][1] == level:
            curve[r] = float(pts[0][0])
    return curve


# ---- lossy compression: the exact 8 x 8 block codec (not in the reference's script) --------------------------------------------------
# An input that went through a lossy block-transform codec (teleradiology, archive migration, detector firmware that compresses before
# processing) is a perturbation every deployed processor meets, and a multi-scale contrast amplifier is the kind of processor that turns
# invisible 8 x 8 blocking into visible structure. block_codec is an integer DCT codec stated so that a device can reproduce it bit for
# bit: it is the contract of musica_alter_codec and musica_sim_codec_reference (include/musica.h).

# M[0][x] = 512, M[u][x] = rint(512 sqrt 2 cos((2x + 1) u pi / 16)): 1024 sqrt 2 (about 1448) times the orthonormal 8-point DCT-II, rounded,
# as literals; a forward and a backward pass together are scaled by 2^21, which the shifts of 10 and 11 bits take out
CODEC_M = np.array([[512, 512, 512, 512, 512, 512, 512, 512],
                    [710, 602, 402, 141, -141, -402, -602, -710],
                    [669, 277, -277, -669, -669, -277, 277, 669],
                    [602, -141, -710, -402, 402, 710, 141, -602],
                    [512, -512, -512, 512, 512, -512, -512, 512],
                    [402, -710, 141, 602, -602, -141, 710, -402],
                    [277, -669, 669, -277, -277, 669, -669, 277],
                    [141, -402, 602, -710, 710, -602, 402, -141]], dtype=np.int64)
# The luminance quantisation table of ITU-T T.81 (JPEG), Annex K, table K.1, indexed [v][u]
CODEC_K = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
                    [12, 12, 14, 19, 26, 58, 60, 55],
                    [14, 13, 16, 24, 40, 57, 69, 56],
                    [14, 17, 22, 29, 51, 87, 80, 62],
                    [18, 22, 37, 56, 68, 109, 103, 77],
                    [24, 35, 55, 64, 81, 104, 113, 92],
                    [49, 64, 78, 87, 103, 121, 120, 101],
                    [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.int64)
CODECS = (16, 64, 256, 1024, 4096)   # the study's DC steps: 4096 is the 8-bit quality-50 table at 16-bit scale


def codec_table(s):
    """The study's quantiser table of DC step s: clip((K s + 8) >> 4, 1, 65535) with K the Annex K luminance table, so Q[0][0] = s exactly
    (s in 1 .. 65535, else ValueError). An (8, 8) uint16 array indexed [v][u]."""
    s = int(s)
    if not 1 <= s <= 65535:
        raise ValueError("codec step %d is not in 1 .. 65535" % s)
    return np.clip((CODEC_K * s + 8) >> 4, 1, 65535).astype(np.uint16)


def codec_table8(table):
    """The table of a processed 8-bit plane that goes with a 16-bit table: max(1, (table + 128) >> 8)."""
    return np.maximum(1, (mp.codec_table_words(table).astype(np.int64) + 128) >> 8).astype(np.uint16)


def _codec_rs(t, s):
    return (t + (1 << (s - 1))) >> s   # numpy's >> of a signed integer is arithmetic


def codec_blocks(X, Q):
    """block_codec's arithmetic on blocks X[..., y, x] of level-shifted int64 pixels with the table Q[v][u]: the stages A, F, F', A' and
    X' (before the level shift back and the last clamp) and the raw products X M^T, M A, M^T F' and A' M, whose bounds are the int32
    contract. A dict of int64 arrays."""
    M = CODEC_M
    p1 = X @ M.T                                       # [y][u]
    A = _codec_rs(p1, 10)
    p2 = M @ A                                         # [v][u]
    F = _codec_rs(p2, 11)
    Fq = np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q) * Q
    p3 = M.T @ Fq                                      # [y][u]
    A2 = np.clip(_codec_rs(p3, 10), -(1 << 18), (1 << 18) - 1)
    p4 = A2 @ M                                        # [y][x]
    return {"XMt": p1, "A": A, "MA": p2, "F": F, "Fq": Fq, "MtF": p3, "A2": A2, "A2M": p4, "X2": _codec_rs(p4, 11)}


def block_codec(plane, table, origin=(0, 0)):
    """The exact 8 x 8 integer block codec of a square 2-D uint16 (bits = 16) or uint8 (bits = 8) plane of side n. table: 8 x 8 integers
    1 .. 65535, the quantiser step per coefficient, indexed [v][u] with v the vertical frequency. origin = (oy, ox), each 0 .. 7, places
    the plane on a larger grid: blocks start at x = -ox and y = -oy (mod 8). A block that sticks out of the plane is completed by edge
    replication, as JPEG does; only in-plane pixels are returned. Per block everything is int32-sized integers, with
    rs(t, s) = (t + 2^(s - 1)) >> s (arithmetic shift) and M = CODEC_M:
        X  = v - 2^(bits - 1)
        A  = rs(X M^T, 10)                           rows        |X M^T| <= 2^27
        F  = rs(M A, 11)                             columns     |M A| <= 2^29, |F| <= 2^18 (the orthonormal DCT, DC = 8 mean exactly)
        q  = sign(F) ((|F| + (Q >> 1)) div Q)        halves away from zero
        F' = q Q                                     |F'| <= 2^18 + 32767
        A' = clamp(rs(M^T F', 10), -2^18, 2^18 - 1)  |M^T F'| <= 3825 (2^18 + 32767) < 2^31; the clamp is part of the contract
        X' = rs(A' M, 11)                            |A' M| <= 2^30
        out = clamp(X' + 2^(bits - 1), 0, 2^bits - 1)
    A constant block comes back exactly whenever Q[0][0] divides 8 X; M departs from orthogonality by 0.06 %, so Q = 1 is not lossless.
    The result has the input's dtype. ValueError for anything else."""
    plane = np.asarray(plane)
    if plane.ndim != 2 or plane.shape[0] != plane.shape[1] or plane.dtype not in (np.uint16, np.uint8) or not plane.size:
        raise ValueError("block_codec needs a non-empty square 2-D uint16 or uint8 plane, got %r %s" % (plane.shape, plane.dtype))
    Q = mp.codec_table_words(table).astype(np.int64)
    try:
        oy, ox = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise ValueError("a codec origin is (oy, ox), got %r" % (origin,))
    if not (0 <= oy <= 7 and 0 <= ox <= 7):
        raise ValueError("codec origin %r is not in 0 .. 7" % (origin,))
    n = plane.shape[0]
    bits = 8 * plane.dtype.itemsize
    half = 1 << (bits - 1)
    by, bx = (n + oy + 7) // 8, (n + ox + 7) // 8
    grid = np.pad(plane.astype(np.int64), ((oy, 8 * by - n - oy), (ox, 8 * bx - n - ox)), mode="edge")
    X = grid.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - half
    out = codec_blocks(X, Q)["X2"].transpose(0, 2, 1, 3).reshape(8 * by, 8 * bx) + half
    return np.clip(out, 0, (1 << bits) - 1)[oy:oy + n, ox:ox + n].astype(plane.dtype)


# ---- lattice sums: a comparison folded by the position modulo a period (not in the reference's script) --------------------------------
# Blocking is a lattice artefact, and so is the shift variance of the decimated pyramid, with periods 2, 4 .. 32 on the raw grid. No other
# metric conditions on a pixel's position modulo a period. lattice_statistics is the contract of musica_sim_lattice (include/musica.h),
# whose tables are bit-identical to it; lattice_summary is what the study reports of the integers, one function for every path.

LATTICE_PERIODS = (2, 4, 8, 16, 32)


def lattice_statistics(a, b, queries, period, origin):
    """What musica_sim_lattice returns for every query (ax, ay, bx, by, w, h), w, h >= 2, of two 2-D uint8 planes (side a, side b): a
    list of (P, P, 8) uint64 tables, P = period in LATTICE_PERIODS, origin o in 0 .. P - 1. The sums run over the query's pixels (i, j)
    with i < w - 1 and j < h - 1, so that every counted pixel has a right and a lower neighbour inside the region; the class of a pixel
    is [(ay + j + o) mod P][(ax + i + o) mod P], side a's position on the raw grid. Per class (processing.LATTICE_FIELDS): n, sum a,
    sum b, sum (a - b)^2, sum (a[i + 1] - a[i])^2, the same of b, sum (a[j + 1] - a[j])^2, the same of b."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("lattice_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    P, o = mp.lattice_period(period, origin)
    res = []
    for region in queries:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 2 or h < 2 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is smaller than 2 x 2 or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        pa, pb = a[ay:ay + h, ax:ax + w].astype(np.int64), b[by:by + h, bx:bx + w].astype(np.int64)
        ca, cb = pa[:-1, :-1], pb[:-1, :-1]
        fields = [np.ones_like(ca), ca, cb, (ca - cb) ** 2, (pa[:-1, 1:] - ca) ** 2, (pb[:-1, 1:] - cb) ** 2, (pa[1:, :-1] - ca) ** 2, (pb[1:, :-1] - cb) ** 2]
        cls = (((ay + o + np.arange(h - 1)) % P)[:, None] * P + ((ax + o + np.arange(w - 1)) % P)[None, :]).ravel()
        table = np.stack([_int_bincount(cls, f.ravel(), P * P) for f in fields], axis=1)
        res.append(table.reshape(P, P, len(fields)).astype(np.uint64))
    return res


def _int_bincount(classes, values, count):
    """sum of the int64 `values` per class, exactly (np.bincount's weights are doubles)."""
    out = np.zeros(count, dtype=np.int64)
    np.add.at(out, classes, values)
    return out


def lattice_fold(table, period):
    """A (P, P, 8) lattice table folded by phase mod `period` (a divisor of P): the table of that period with the origin o mod period."""
    t = np.asarray(table)
    P = t.shape[0]
    if t.ndim != 3 or t.shape[1] != P or P % int(period):
        raise ValueError("a lattice table is (P, P, 8) and folds to a divisor of P, got %r to %r" % (t.shape, period))
    p = int(period)
    return t.reshape(P // p, p, P // p, p, t.shape[2]).sum(axis=(0, 2), dtype=t.dtype)


LATTICE_AXIS_KEYS = ("step_a", "step_b", "amplified", "phase_mse")   # lattice_summary's numbers per axis; "periodic" beside the axes


def lattice_summary(table):
    """What the study reports of a comparison's lattice sums, from lattice_statistics' (or musica_sim_lattice's) exact integers of ONE
    query: one function for every study path. With the table summed over the other axis' phases, per axis ("x": the column phase and
    the horizontal steps, "y": the row phase and the vertical steps):
        step_a, step_b  the mean squared step across the lattice line (phase P - 1 -> 0) over the mean squared step at the other phases
        amplified       step_a / step_b
        phase_mse       {p: the largest over the mean of the p per-phase mse} for every period p | P, p >= 2, the table folded to p
    and "periodic": the share of sum (d - mean d)^2, d = a - b, carried by the class means of d over the P^2 classes. A quotient with
    a zero denominator is None. Every float is one division of exact integers (the phase_mse mean: of exact fractions). No threshold is
    fixed here: these are findings."""
    t = np.asarray(table)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[0] not in LATTICE_PERIODS or t.shape[2] != len(mp.LATTICE_FIELDS) or t.dtype.kind not in "iu":
        raise ValueError("a lattice table is (P, P, %d) integers with P in %r, got %r %s" % (len(mp.LATTICE_FIELDS), LATTICE_PERIODS, t.shape, t.dtype))
    P = t.shape[0]
    v = [[[int(x) for x in cell] for cell in row] for row in t]
    out = {}
    for axis, name, fa, fb in ((1, "x", 4, 5), (0, "y", 6, 7)):
        # per phase along the axis: every field summed over the other axis
        line = [[sum((v[k][p] if axis == 1 else v[p][k])[f] for k in range(P)) for f in range(len(mp.LATTICE_FIELDS))] for p in range(P)]
        steps = {}
        for key, f in (("step_a", fa), ("step_b", fb)):
            across = (line[P - 1][f], line[P - 1][0])
            others = (sum(line[p][f] for p in range(P - 1)), sum(line[p][0] for p in range(P - 1)))
            steps[key] = (across[0] * others[1], across[1] * others[0])   # the quotient of the two means as one fraction
        entry = {k: (n / d if d else None) for k, (n, d) in steps.items()}
        (na, da), (nb, db) = steps["step_a"], steps["step_b"]
        entry["amplified"] = (na * db) / (da * nb) if da and db and nb else None
        entry["phase_mse"] = {}
        p = 2
        while p <= P:
            folded = [(sum(line[k][3] for k in range(P) if k % p == ph), sum(line[k][0] for k in range(P) if k % p == ph)) for ph in range(p)]
            if any(n == 0 for _, n in folded):
                entry["phase_mse"][p] = None
            else:
                mses = [Fraction(s, n) for s, n in folded]
                mean = sum(mses) / p
                entry["phase_mse"][p] = float(max(mses) / mean) if mean else None
            p *= 2
        out[name] = entry
    cells = [c for row in v for c in row]
    n = sum(c[0] for c in cells)
    sd = sum(c[1] - c[2] for c in cells)
    sdd = sum(c[3] for c in cells)
    # n times the sums of squares, so that everything stays an integer: total = n sum d^2 - (sum d)^2
    total = n * sdd - sd * sd
    between = sum((Fraction((c[1] - c[2]) ** 2, c[0]) for c in cells if c[0]), Fraction(0)) * n - sd * sd
    out["periodic"] = float(between / total) if total else None
    return out


def lattice_row(table):
    """A row's *_lattice value: lattice_summary's dict and "table", the (P, P, 8) exact integers as nested lists."""
    return dict(lattice_summary(table), table=np.asarray(table).astype(np.uint64).tolist())


# ---- blobs: the connected components of a comparison's change mask (not in the reference's script) ------------------------------------
# Every other metric sums a comparison over a set chosen before the pixels are looked at; 300 isolated flips and one 300-pixel streak of
# the same |a - b| are the same to all of them. blob_statistics labels the mask |a - b| > threshold and is the contract of
# musica_sim_blobs (include/musica.h), whose tables, largest component and label planes are bit-identical to it; blob_summary is what the
# study reports of the integers, one function for every path.

BLOB_STRUCTURES = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool), 8: np.ones((3, 3), dtype=bool)}
BLOB_CLUSTERED_CLASS = 4   # components of 16 pixels at least: blob_summary's "clustered"


def blob_statistics(a, b, queries, threshold, connectivity=8):
    """What musica_sim_blobs returns for every query (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side b): a list
    of dicts. The mask of a query is |a - b| > threshold (processing.blob_threshold: 0 .. 254) over its pixels; connectivity 4 or 8; a
    pixel of the region connects only to pixels of the region (scipy.ndimage.label with the matching structure, then integers only).
    The canonical label of a component is 1 + the row-major index y w + x, within the region, of its first pixel, 0 off the mask:
    nothing depends on scipy's numbering. Per query:
      "table"       (BLOB_CLASSES, 6) uint64, the class of a component of n pixels being n.bit_length() - 1; per class the
                    processing.BLOB_FIELDS components, pixels, sum_d = sum |a - b|, sum_dd = sum (a - b)^2, box_area = the sum of the
                    bounding boxes' areas, border = the components with a pixel on the region's outline
      "pixels"      w h;  "changed": the mask's pixels;  "components"      (Python ints)
      "largest"     the dict n, first, x0, y0, x1, y1, sum_dd of the largest component (first: its first pixel's row-major index; the
                    box inclusive; of equal sizes the smaller first wins); all 0 where nothing changed
      "labels"      the (h, w) uint32 plane of the canonical labels."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("blob_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    t = mp.blob_threshold(threshold)
    if connectivity not in BLOB_STRUCTURES:
        raise ValueError("connectivity %r is neither 4 nor 8" % (connectivity,))
    res = []
    for region in queries:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        d = np.abs(a[ay:ay + h, ax:ax + w].astype(np.int64) - b[by:by + h, bx:bx + w].astype(np.int64))
        mask = d > t
        numbered, count = ndimage.label(mask, structure=BLOB_STRUCTURES[connectivity])
        table = np.zeros((mp.BLOB_CLASSES, len(mp.BLOB_FIELDS)), dtype=np.uint64)
        largest = dict.fromkeys(("n", "first", "x0", "y0", "x1", "y1", "sum_dd"), 0)
        labels = np.zeros((h, w), dtype=np.uint32)
        if count:
            at = np.flatnonzero(mask)                     # ascending: the row-major order
            of = numbered.ravel()[at] - 1                 # scipy's number of every mask pixel, from 0
            _, where = np.unique(of, return_index=True)
            first = at[where]                             # per component: its first pixel
            y, x, dm = at // w, at % w, d.ravel()[at]
            n, sd, sdd = (_int_bincount(of, v, count) for v in (np.ones_like(at), dm, dm * dm))
            x0, y0 = np.full(count, w, dtype=np.int64), np.full(count, h, dtype=np.int64)
            x1, y1 = np.zeros(count, dtype=np.int64), np.zeros(count, dtype=np.int64)
            np.minimum.at(x0, of, x)
            np.minimum.at(y0, of, y)
            np.maximum.at(x1, of, x)
            np.maximum.at(y1, of, y)
            border = ((x0 == 0) | (y0 == 0) | (x1 == w - 1) | (y1 == h - 1)).astype(np.int64)
            cls = np.array([int(v).bit_length() - 1 for v in n])
            fields = (np.ones_like(n), n, sd, sdd, (x1 - x0 + 1) * (y1 - y0 + 1), border)
            table = np.stack([_int_bincount(cls, f, mp.BLOB_CLASSES) for f in fields], axis=1).astype(np.uint64)
            k = min(range(count), key=lambda i: (-int(n[i]), int(first[i])))
            largest = {"n": int(n[k]), "first": int(first[k]), "x0": int(x0[k]), "y0": int(y0[k]), "x1": int(x1[k]), "y1": int(y1[k]), "sum_dd": int(sdd[k])}
            labels.ravel()[at] = (first[of] + 1).astype(np.uint32)
        res.append({"table": table, "pixels": w * h, "changed": int(mask.sum()), "components": int(count), "largest": largest, "labels": labels})
    return res


BLOB_KEYS = ("components", "changed", "isolated", "clustered", "largest", "largest_dd", "mean_size", "fill", "border")   # blob_summary's numbers; "largest_box", "class_components" and "class_pixels" beside them


def blob_summary(stats):
    """What the study reports of a comparison's components, from ONE dict of blob_statistics (or sim_blobs): one function for every
    study path. "components": their number; then the shares, each one division of exact integers and None where nothing changed:
        changed      the mask's pixels over the region's (0.0 where nothing changed, None only for an empty region)
        isolated     the pixels of single-pixel components over the changed ones
        clustered    the pixels of components of 16 pixels at least over the changed ones
        largest      the largest component's pixels over the changed ones;  largest_dd: its sum (a - b)^2 over the mask's
        mean_size    the changed pixels over the components
        fill         the changed pixels over the sum of the components' box areas
        border       the components with a pixel on the region's outline over the components
    and "largest_box" [x0, y0, x1, y1] (None where nothing changed), "class_components" and "class_pixels", BLOB_CLASSES ints each."""
    t = np.asarray(stats["table"])
    if t.shape != (mp.BLOB_CLASSES, len(mp.BLOB_FIELDS)) or t.dtype.kind not in "iu":
        raise ValueError("a blob table is (%d, %d) integers, got %r %s" % (mp.BLOB_CLASSES, len(mp.BLOB_FIELDS), t.shape, t.dtype))
    v = [[int(x) for x in row] for row in t]
    comps, px, sdd, area, border = (sum(row[f] for row in v) for f in (0, 1, 3, 4, 5))
    big = stats["largest"]
    if px != int(stats["changed"]) or comps != int(stats["components"]):
        raise ValueError("the table's classes add up to %d pixels in %d components, the statistics say %d in %d" % (px, comps, stats["changed"], stats["components"]))
    share = lambda n, d: n / d if d else None
    return {"components": comps, "changed": share(px, int(stats["pixels"])), "isolated": share(v[0][1], px),
            "clustered": share(sum(row[1] for row in v[BLOB_CLUSTERED_CLASS:]), px), "largest": share(int(big["n"]), px),
            "largest_dd": share(int(big["sum_dd"]), sdd), "mean_size": share(px, comps), "fill": share(px, area), "border": share(border, comps),
            "largest_box": [int(big[k]) for k in ("x0", "y0", "x1", "y1")] if px else None,
            "class_components": [row[0] for row in v], "class_pixels": [row[1] for row in v]}


def blob_row(stats):
    """A row's *_blobs value: blob_summary's dict and "table", the (BLOB_CLASSES, 6) exact integers as nested lists."""
    return dict(blob_summary(stats), table=np.asarray(stats["table"]).astype(np.uint64).tolist())


# ---- spectrum: the exact Walsh transforms of a comparison (not in the reference's script) ---------------------------------------------
# MUSICA amplifies bands, so its transfer function is a gain per band. The grating rows measure it on inserted sine patches, the scales on
# low-pass pooled planes without orientation; the transform-domain sums of a comparison give, for the image itself, the gain, the coherence
# and the share of the error per band and orientation. A Fourier transform cannot be exact integers; the Walsh-Hadamard transform can, and
# its octave bands are the Haar subbands. spectrum_statistics is the contract of musica_sim_spectrum (include/musica.h), whose tables are
# bit-identical to it; spectrum_summary is what the study reports of the integers, one function for every path.

_WALSH = {}


def walsh_matrix(tile):
    """The T x T Walsh matrix in sequency order, int64: row s is the row of the Sylvester Hadamard matrix (scipy.linalg.hadamard) with
    exactly s sign changes. T as processing.spectrum_tile takes it."""
    T = mp.spectrum_tile(tile)
    if T not in _WALSH:
        from scipy.linalg import hadamard
        H = hadamard(T).astype(np.int64)
        changes = (H[:, 1:] != H[:, :-1]).sum(axis=1)
        if sorted(changes.tolist()) != list(range(T)):
            raise AssertionError("the sign changes of the Sylvester rows of order %d are not 0 .. %d" % (T, T - 1))
        _WALSH[T] = (H[np.argsort(changes)], np.argsort(changes))
    return _WALSH[T][0]


def _hadamard_axis(x, axis):
    """The butterflies of the Sylvester Hadamard transform along `axis` (a power of two long) of an int64 array: natural order."""
    x = np.moveaxis(x, axis, -1)
    shape, T = x.shape, x.shape[-1]
    h = 1
    while h < T:
        y = x.reshape(shape[:-1] + (T // (2 * h), 2, h))
        x = np.stack([y[..., 0, :] + y[..., 1, :], y[..., 0, :] - y[..., 1, :]], axis=-2).reshape(shape)
        h *= 2
    return np.moveaxis(x, -1, axis)


def spectrum_statistics(a, b, queries, tile):
    """What musica_sim_spectrum returns for every query (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side b): a
    list of dicts. A region holds tx = w // T by ty = h // T whole tiles of T x T pixels, T = tile in 8, 16, 32, 64, anchored at its
    first pixel on either side; the remainder columns and rows are not counted. Per tile A = W a W^T and B = W b W^T in integers
    (W = walsh_matrix(T)); "table" is the (T, T, 3) int64 array, indexed [row sequency][column sequency], of the sums over the tiles
    of A^2, B^2 and A B (processing.SPECTRUM_FIELDS), all zeros where "tiles" = tx ty is 0. The butterflies here are a fast form of the
    two matrix products; tests/test_spectrum_restatement.py holds them to the literal ones."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("spectrum_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    T = mp.spectrum_tile(tile)
    walsh_matrix(T)
    order = _WALSH[T][1]   # the natural index of every sequency
    res = []
    for region in queries:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        tx, ty = w // T, h // T
        table = np.zeros((T, T, len(mp.SPECTRUM_FIELDS)), dtype=np.int64)
        if tx and ty:
            coeff = []
            for plane, x0, y0 in ((a, ax, ay), (b, bx, by)):
                tiles = plane[y0:y0 + ty * T, x0:x0 + tx * T].astype(np.int64).reshape(ty, T, tx, T)
                coeff.append(_hadamard_axis(_hadamard_axis(tiles, 1), 3)[:, order][:, :, :, order])
            A, B = coeff
            table[:, :, 0], table[:, :, 1], table[:, :, 2] = (A * A).sum(axis=(0, 2)), (B * B).sum(axis=(0, 2)), (A * B).sum(axis=(0, 2))
        res.append({"table": table, "tiles": tx * ty})
    return res


SPECTRUM_BAND_KEYS = ("gain", "coherence", "error")   # spectrum_summary's numbers of a band pair and of a radial band
SPECTRUM_KEYS = ("slope", "horizontal", "vertical", "diagonal", "dc", "ac_gain", "ac_coherence")   # ... and of the whole table; "bands" and "radial" beside them


def _spectrum_band(aa, bb, ab, total):
    """gain = sqrt(sum A^2 / sum B^2), coherence = sum A B / sqrt(sum A^2 sum B^2), error = the share of sum (A - B)^2 in `total`."""
    return {"gain": math.sqrt(aa / bb) if bb else None, "coherence": ab / math.sqrt(aa * bb) if aa and bb else None,
            "error": (aa + bb - 2 * ab) / total if total else 0.0}


def spectrum_summary(table, tiles, tile):
    """What the study reports of a comparison's Walsh sums, from spectrum_statistics' (or musica_sim_spectrum's) exact integers of ONE
    query: one function for every study path; None where `tiles` is 0. The band of a sequency s is s.bit_length(): 0 (DC), 1 .. log2 T
    per axis, the octaves of the Haar subbands. With the three sums added up over a set of coefficients,
        gain        sqrt(sum A^2 / sum B^2): what side a has of the band over what side b has; None where sum B^2 is 0
        coherence   sum A B / sqrt(sum A^2 sum B^2): 1 where a's band is b's times a positive number; None where either sum is 0
        error       the set's share of sum (A - B)^2 over the whole table (by Parseval T^2 times the sum of squared differences of the
                    tiled area); 0.0 everywhere where the sides are equal
    "bands"[cy][cx] has the three for the band pair (row band cy, column band cx), "radial"[r] for the pairs with max(cy, cx) = r.
    "slope": the least-squares slope of log2 gain on r over the AC radial bands r >= 1 that have a gain above 0 (None with fewer than
    two): the octave-to-octave tilt of the transfer function. "horizontal", "vertical", "diagonal", "dc": the error shares of the pairs
    with cx > cy (finer along a row than down a column), cx < cy, cx = cy > 0, and of the DC coefficient. "ac_gain", "ac_coherence":
    gain and coherence over every coefficient but DC. Every share and quotient is one division of exact integers."""
    T = mp.spectrum_tile(tile)
    t = np.asarray(table)
    if t.shape != (T, T, len(mp.SPECTRUM_FIELDS)) or t.dtype.kind not in "iu":
        raise ValueError("a spectrum table of tile %d is (%d, %d, %d) integers, got %r %s" % (T, T, T, len(mp.SPECTRUM_FIELDS), t.shape, t.dtype))
    if not int(tiles):
        return None
    bands = T.bit_length()   # 0 .. log2 T
    v = t.astype(np.int64)   # sum A B is signed: a uint64 table holds it in two's complement
    sums = [[[0, 0, 0] for _ in range(bands)] for _ in range(bands)]
    for sv in range(T):
        for su in range(T):
            cell = sums[sv.bit_length()][su.bit_length()]
            for f in range(3):
                cell[f] += int(v[sv, su, f])
    pairs = [(cy, cx) for cy in range(bands) for cx in range(bands)]
    over = lambda keep: tuple(sum(sums[cy][cx][f] for cy, cx in pairs if keep(cy, cx)) for f in range(3))   # noqa: E731
    err = lambda s: s[0] + s[1] - 2 * s[2]   # noqa: E731
    total = err(over(lambda cy, cx: True))
    share = lambda keep: err(over(keep)) / total if total else 0.0   # noqa: E731
    out = {"bands": [[_spectrum_band(*sums[cy][cx], total) for cx in range(bands)] for cy in range(bands)],
           "radial": [_spectrum_band(*over(lambda cy, cx, r=r: max(cy, cx) == r), total) for r in range(bands)]}
    points = [(r, math.log2(band["gain"])) for r, band in enumerate(out["radial"]) if r >= 1 and band["gain"]]
    if len(points) >= 2:
        mx, my = sum(x for x, _ in points) / len(points), sum(y for _, y in points) / len(points)
        out["slope"] = sum((x - mx) * (y - my) for x, y in points) / sum((x - mx) ** 2 for x, _ in points)
    else:
        out["slope"] = None
    out["horizontal"], out["vertical"] = share(lambda cy, cx: cx > cy), share(lambda cy, cx: cx < cy)
    out["diagonal"], out["dc"] = share(lambda cy, cx: cx == cy and cx > 0), share(lambda cy, cx: cx == 0 and cy == 0)
    ac = _spectrum_band(*over(lambda cy, cx: cx > 0 or cy > 0), total)
    out["ac_gain"], out["ac_coherence"] = ac["gain"], ac["coherence"]
    return out


def spectrum_row(stats, tile):
    """A row's *_spectrum value from ONE dict of spectrum_statistics (or sim_spectrum): spectrum_summary's dict, "tile", "tiles" and
    "table", the (T, T, 3) exact integers as nested lists; None where the region holds no tile."""
    summary = spectrum_summary(stats["table"], stats["tiles"], tile)
    if summary is None:
        return None
    return dict(summary, tile=int(tile), tiles=int(stats["tiles"]), table=np.asarray(stats["table"]).astype(np.int64).tolist())


# ---- the texture of a comparison: gray-level co-occurrence matrices ------------------------------------------------------------------
# Did the texture of the image survive? The second-order gray-level statistics of Haralick, Shanmugam and Dinstein (1973), the terms
# in which radiomics reports the stability of features under processing. cooccurrence_statistics is the contract of
# musica_sim_cooccurrence (include/musica.h), whose tables are bit-identical to it; cooccurrence_summary is what the study reports of
# the integers, one function for every path.

COOCCURRENCE_DIRECTIONS = (0, 45, 90, 135)   # degrees; the offset of direction i at distance d is cooccurrence_offsets(d)[i]


def cooccurrence_offsets(d):
    """The offsets (dx, dy) of the four directions at distance d: 0 (d, 0), 45 (d, d), 90 (0, d), 135 (-d, d); y runs down."""
    return ((d, 0), (d, d), (0, d), (-d, d))


def cooccurrence_statistics(a, b, regions, levels, distances):
    """What musica_sim_cooccurrence returns for every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side
    b): a list of dicts. The level of a pixel v is v >> (8 - log2 G), G = levels in 8, 16, 32, 64 (processing.cooccurrence_levels);
    distances: 1 .. 4 distinct ascending d in 1 .. 16 (processing.cooccurrence_distances). A pair (p, p + offset) counts on a side
    where both pixels lie inside the region on that side, once, in T[level(p)][level(p + offset)]: nothing is symmetrised.
    "table": the (D, 4, 2, G, G) uint32 array [distance][direction][side a = 0, b = 1] (a region has fewer than 2^32 pairs);
    "pairs": the (D, 4) uint64 array (w - |dx|) (h - dy), 0 where the region is too small for the offset: its tables are then zero."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("cooccurrence_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    G, ds = mp.cooccurrence_levels(levels), mp.cooccurrence_distances(distances)
    shift = 8 - (G.bit_length() - 1)
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        sides = ((a[ay:ay + h, ax:ax + w] >> shift).astype(np.int64), (b[by:by + h, bx:bx + w] >> shift).astype(np.int64))
        table = np.zeros((len(ds), 4, 2, G, G), dtype=np.uint32)
        pairs = np.zeros((len(ds), 4), dtype=np.uint64)
        for k, d in enumerate(ds):
            for i, (dx, dy) in enumerate(cooccurrence_offsets(d)):
                cols, rows = w - abs(dx), h - dy
                if cols <= 0 or rows <= 0:
                    continue
                pairs[k, i] = cols * rows
                x0 = max(0, -dx)   # the first pixels' first column
                for s, lv in enumerate(sides):
                    first, second = lv[:rows, x0:x0 + cols], lv[dy:dy + rows, x0 + dx:x0 + dx + cols]
                    table[k, i, s] = np.bincount((first * G + second).ravel(), minlength=G * G).reshape(G, G)
        res.append({"table": table, "pairs": pairs})
    return res


COOCCURRENCE_FEATURES = ("contrast", "dissimilarity", "homogeneity", "energy", "entropy", "correlation")   # cooccurrence_features' numbers


def cooccurrence_features(C):
    """Haralick's features of ONE symmetric G x G matrix C of non-negative integers with a positive sum N, P = C / N:
        contrast sum (i - j)^2 P, dissimilarity sum |i - j| P, homogeneity sum P / (1 + (i - j)^2), energy sum P^2,
        entropy -sum P log2 P (bits), correlation sum (i - mu)(j - mu) P / var, 1.0 where the side is flat (var = 0: skimage's convention).
    The sums over |i - j| = k, sum C^2, sum i j C and the marginal's moments are exact integers and every sum of quotients is
    math.fsum's correctly rounded one, so a value does not depend on the order of the cells: the negative and the transposed matrix
    give the same bits."""
    G = len(C)
    C = [[int(v) for v in row] for row in C]
    N = sum(map(sum, C))
    by_k = [0] * G
    squares = moment = 0
    for i in range(G):
        for j in range(G):
            by_k[abs(i - j)] += C[i][j]
            squares += C[i][j] * C[i][j]
            moment += i * j * C[i][j]
    s1 = sum(i * sum(C[i]) for i in range(G))
    s2 = sum(i * i * sum(C[i]) for i in range(G))
    var = N * s2 - s1 * s1
    return {"contrast": sum(k * k * n for k, n in enumerate(by_k)) / N, "dissimilarity": sum(k * n for k, n in enumerate(by_k)) / N,
            "homogeneity": math.fsum(n / (1 + k * k) for k, n in enumerate(by_k)) / N, "energy": squares / (N * N),
            "entropy": math.fsum(c / N * math.log2(N / c) for row in C for c in row if c),
            "correlation": (N * moment - s1 * s1) / var if var else 1.0}


def _cooccurrence_divergence(Ca, Cb):
    """The Jensen-Shannon divergence in bits of Pa = Ca / N and Pb = Cb / N (the two sides of a region have the same pairs, so one N):
    (sum Ca log2(2 Ca / (Ca + Cb)) + sum Cb log2(2 Cb / (Ca + Cb))) / 2 N, exactly 0.0 where the matrices are equal."""
    N = sum(int(v) for row in Ca for v in row)
    terms = []
    for ra, rb in zip(Ca, Cb):
        for x, y in zip(ra, rb):
            x, y = int(x), int(y)
            if x != y:
                terms.extend(c * math.log2(2 * c / (x + y)) for c in (x, y) if c)
    return max(0.0, math.fsum(terms) / (2 * N))


def cooccurrence_summary(table, pairs, levels, distances):
    """What the study reports of a comparison's co-occurrence tables, from cooccurrence_statistics' (or musica_sim_cooccurrence's)
    exact integers of ONE region: one function for every study path; None where no distance has a pair. Per side and distance the
    symmetric, direction-summed matrix C = sum over the directions of (T + T^T), P = C / sum C. "distances"[k] is None where distance
    k has no pair in any direction, else
        "distance", "pairs"   d and the pairs of its four directions together
        "a", "b"              cooccurrence_features of the side's C, and "anisotropy": (max - min) / mean of the contrast of
                              T + T^T over the directions that have pairs, 0.0 where the mean is 0 (a flat side)
        "difference"          a's feature minus b's, per feature, and of the anisotropy
        "divergence"          the Jensen-Shannon divergence of P_a and P_b, in bits (0 .. 1)
    "divergence": the largest over the distances."""
    G, ds = mp.cooccurrence_levels(levels), mp.cooccurrence_distances(distances)
    t, n = np.asarray(table), np.asarray(pairs)
    if t.shape != (len(ds), 4, 2, G, G) or t.dtype.kind not in "iu" or n.shape != (len(ds), 4):
        raise ValueError("the co-occurrence tables of %d levels and %d distances are (%d, 4, 2, %d, %d) integers with (%d, 4) pairs, got %r %s and %r"
                         % (G, len(ds), len(ds), G, G, len(ds), t.shape, t.dtype, n.shape))
    t = t.astype(np.int64)
    out = []
    for k, d in enumerate(ds):
        have = [i for i in range(4) if int(n[k, i])]
        if not have:
            out.append(None)
            continue
        entry = {"distance": d, "pairs": sum(int(n[k, i]) for i in have)}
        matrices = []
        for s, side in enumerate("ab"):
            sym = [t[k, i, s] + t[k, i, s].T for i in range(4)]
            C = sum(sym[i] for i in have).tolist()
            matrices.append(C)
            entry[side] = cooccurrence_features(C)
            contrasts = [cooccurrence_features(sym[i].tolist())["contrast"] for i in have]
            mean = math.fsum(contrasts) / len(contrasts)
            entry[side]["anisotropy"] = (max(contrasts) - min(contrasts)) / mean if mean else 0.0
        entry["difference"] = {f: entry["a"][f] - entry["b"][f] for f in COOCCURRENCE_FEATURES + ("anisotropy",)}
        entry["divergence"] = _cooccurrence_divergence(*matrices)
        out.append(entry)
    if all(e is None for e in out):
        return None
    return {"distances": out, "divergence": max(e["divergence"] for e in out if e is not None)}


def texture_row(stats, levels, distances):
    """A row's *_texture value from ONE dict of cooccurrence_statistics (or sim_cooccurrence): cooccurrence_summary's dict, "levels",
    "distance_list" and "pairs", the (D, 4) exact counts as nested lists; None where no distance has a pair. The tables themselves, up to
    131072 words a comparison, are not kept in the row."""
    summary = cooccurrence_summary(stats["table"], stats["pairs"], levels, distances)
    if summary is None:
        return None
    return dict(summary, levels=int(levels), distance_list=[int(d) for d in mp.cooccurrence_distances(distances)],
                pairs=[[int(v) for v in row] for row in np.asarray(stats["pairs"])])


# ---- the sizes of a comparison: the granulometry -----------------------------------------------------------------------------------------
# Which object sizes became brighter or darker, and by how much? The granulometry of mathematical morphology (Matheron 1975; the pattern
# spectrum of Maragos 1989): openings and closings by a growing square sieve the bright and the dark structures by size.
# granulometry_statistics is the contract of musica_sim_granulometry (include/musica.h), whose tables are bit-identical to it;
# granulometry_summary is what the study reports of the integers, one function for every path.

GRANULOMETRY_POLARITIES = ("bright", "dark")
GRANULOMETRY_FIELDS = ("sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab")   # a table's words
GRANULOMETRY_CLASS_KEYS = ("share_a", "share_b", "gain", "coherence", "mse")
GRANULOMETRY_KEYS = ("mean_side_a", "mean_side_b", "mean_side_shift", "slope", "residue_shift")


def granulometry_opening(f, r):
    """The opening of a 2-D uint8 plane by the (2 r + 1)^2 square clipped to the plane (the plane is its own domain): the erosion is the
    minimum over the clipped square (cval=255), the dilation the maximum (cval=0); r = 0 is the identity."""
    if r == 0:
        return f
    eroded = ndimage.minimum_filter(f, size=2 * r + 1, mode="constant", cval=255)
    return ndimage.maximum_filter(eroded, size=2 * r + 1, mode="constant", cval=0)


def granulometry_closing(f, r):
    """The closing by the same element: the erosion of the dilation; 255 - closing(f) = opening(255 - f)."""
    if r == 0:
        return f
    dilated = ndimage.maximum_filter(f, size=2 * r + 1, mode="constant", cval=0)
    return ndimage.minimum_filter(dilated, size=2 * r + 1, mode="constant", cval=255)


def granulometry_statistics(a, b, regions, radii):
    """What musica_sim_granulometry returns for every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side
    b): a list of dicts. radii: K = 1 .. 8 distinct ascending r_1 < .. < r_K in 1 .. 16 (processing.granulometry_radii), r_0 = 0. The
    region's sub-array is its own domain: nothing outside it is read. "table": the (K + 1, 2, 5) uint64 array
    [class][polarity bright = 0, dark = 1][sum A, sum B, sum A^2, sum B^2, sum A B] over the region's pixels, where for class k < K
    A = opening_{r_k}(a) - opening_{r_k+1}(a) (bright) or closing_{r_k+1}(a) - closing_{r_k}(a) (dark) and for the residue, class K,
    A = opening_{r_K}(a) or 255 - closing_{r_K}(a); B likewise from b. "pixels": w * h."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("granulometry_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    rs = (0,) + mp.granulometry_radii(radii)
    K = len(rs) - 1
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        sides = (np.ascontiguousarray(a[ay:ay + h, ax:ax + w]), np.ascontiguousarray(b[by:by + h, bx:bx + w]))
        table = np.zeros((K + 1, 2, len(GRANULOMETRY_FIELDS)), dtype=np.uint64)
        for p, sieve in enumerate((granulometry_opening, granulometry_closing)):
            planes = [[sieve(f, r).astype(np.int64) for r in rs] for f in sides]
            for k in range(K + 1):
                if k < K:
                    A, B = ((g[k] - g[k + 1]) if p == 0 else (g[k + 1] - g[k]) for g in planes)
                else:
                    A, B = (g[K] if p == 0 else 255 - g[K] for g in planes)
                table[k, p] = [int(A.sum()), int(B.sum()), int((A * A).sum()), int((B * B).sum()), int((A * B).sum())]
        res.append({"table": table, "pixels": w * h})
    return res


def granulometry_summary(table, radii, pixels):
    """What the study reports of a comparison's granulometry, in f64 from granulometry_statistics' (or musica_sim_granulometry's) exact
    integers of ONE region only: one function for every study path. A dict with "bright" and "dark", each
        "classes"          per class k < K a dict: "radius" r_k+1 and "side" 2 r_k+1 + 1, the element that removes the class;
                           "share_a", "share_b": the pattern spectrum, sum A / the sum of sum A over the classes k < K (None where that is 0);
                           "gain" sum A B / sum B^2 (None where sum B^2 is 0); "coherence" sum A B / sqrt(sum A^2 sum B^2) (None where
                           either is 0); "mse" (sum A^2 + sum B^2 - 2 sum A B) / pixels, the band's mean squared difference
        "mean_side_a", "mean_side_b"   the share-weighted mean element side (None without shares), "mean_side_shift" a's minus b's
        "slope"            the least-squares slope of log gain on log side over the classes that have a positive gain, None with fewer
                           than two: negative where small structures gain more
        "residue_shift"    (sum A - sum B) / pixels of the residue class."""
    rs = mp.granulometry_radii(radii)
    K = len(rs)
    t = np.asarray(table)
    if t.shape != (K + 1, 2, len(GRANULOMETRY_FIELDS)) or t.dtype.kind not in "iu":
        raise ValueError("the granulometry table of %d radii is (%d, 2, %d) integers, got %r %s" % (K, K + 1, len(GRANULOMETRY_FIELDS), t.shape, t.dtype))
    pixels = int(pixels)
    if pixels < 1:
        raise ValueError("a granulometry has at least one pixel, got %d" % pixels)
    out = {}
    for p, polarity in enumerate(GRANULOMETRY_POLARITIES):
        words = [[int(v) for v in t[k, p]] for k in range(K + 1)]
        total_a, total_b = sum(w[0] for w in words[:K]), sum(w[1] for w in words[:K])
        classes = []
        for k in range(K):
            sa, sb, saa, sbb, sab = words[k]
            classes.append({"radius": rs[k], "side": 2 * rs[k] + 1,
                            "share_a": sa / total_a if total_a else None, "share_b": sb / total_b if total_b else None,
                            "gain": sab / sbb if sbb else None, "coherence": sab / math.sqrt(saa * sbb) if saa and sbb else None,
                            "mse": (saa + sbb - 2 * sab) / pixels})
        mean_a = math.fsum(c["side"] * c["share_a"] for c in classes) if total_a else None
        mean_b = math.fsum(c["side"] * c["share_b"] for c in classes) if total_b else None
        points = [(math.log(c["side"]), math.log(c["gain"])) for c in classes if c["gain"] is not None and c["gain"] > 0]
        slope = None
        if len(points) >= 2:
            mx, my = math.fsum(x for x, _ in points) / len(points), math.fsum(y for _, y in points) / len(points)
            slope = math.fsum((x - mx) * (y - my) for x, y in points) / math.fsum((x - mx) * (x - mx) for x, _ in points)
        out[polarity] = {"classes": classes, "mean_side_a": mean_a, "mean_side_b": mean_b,
                         "mean_side_shift": mean_a - mean_b if mean_a is not None and mean_b is not None else None, "slope": slope,
                         "residue_shift": (words[K][0] - words[K][1]) / pixels}
    return out


def granulometry_row(stats, radii):
    """A row's *_granulometry value from ONE dict of granulometry_statistics (or sim_granulometry): granulometry_summary's dict, "radii",
    "pixels" and the exact "table" as nested lists."""
    return dict(granulometry_summary(stats["table"], radii, stats["pixels"]), radii=[int(r) for r in mp.granulometry_radii(radii)],
                pixels=int(stats["pixels"]), table=np.asarray(stats["table"]).astype(np.uint64).tolist())


# ---- the contours of a comparison: the distances between the two edge sets -----------------------------------------------------------------
# Are the contours of the output where the contours of the reference are, how far did they move, how many are new and how many are gone?
# gsim, gc and turn compare gradients at the same pixel: a contour that moved by two pixels and one that vanished while another appeared
# elsewhere look alike to them. The edge-detection literature's answer is the distance between the two edge sets (Pratt's figure of merit,
# the chamfer distances, the Hausdorff distance), all from one table: per contour pixel of one side the exact squared Euclidean distance
# to the nearest contour pixel of the other. contour_statistics is the contract of musica_sim_contours (include/musica.h), whose tables
# and planes are bit-identical to it; contour_summary is what the study reports of the integers, one function for every path.

CONTOUR_DIRECTIONS = ("a_to_b", "b_to_a")   # the table's rows: S = E_a, T = E_b (where a's contours lie with respect to b's), then S = E_b, T = E_a
CONTOUR_KEYS = ("contour_a", "contour_b", "density_a", "density_b", "ratio", "fom", "kept", "moved", "lost", "spurious", "hausdorff")
CONTOUR_DIRECTION_KEYS = ("found", "far", "mean", "median", "p95")
CONTOUR_FOM_SCALE = 9        # Pratt's figure of merit: 1 / (1 + d^2 / 9), Pratt's alpha = 1 / 9
CONTOUR_KEPT_D2 = 2          # a contour pixel is "kept" where the other side has one among its eight neighbours or at its place


def contour_mask(p, threshold):
    """The contour E of a 2-D uint8 plane, which is its own domain, as a bool plane: the strength M = gx^2 + gy^2 of sobel_gradients
    over the interior 1 <= x <= w - 2, 1 <= y <= h - 2 and 0 everywhere else (a plane with a side below 3 has no contour); a pixel is
    horizontal where |gx| >= |gy|, else vertical; `before` / `after` are M(x - 1, y) / M(x + 1, y) of a horizontal pixel and
    M(x, y - 1) / M(x, y + 1) of a vertical one; E = M >= threshold and M > before and M >= after: non-maximum suppression along the
    axis, on a plateau of equal strengths the left or upper pixel is the contour."""
    tau = mp.contour_threshold(threshold)
    p = np.asarray(p)
    h, w = p.shape
    M = np.zeros((h + 2, w + 2), dtype=np.int64)   # M with a frame of zeros: pixel (x, y) at [y + 1][x + 1]
    horizontal = np.ones((h, w), dtype=bool)
    if w >= 3 and h >= 3:
        gx, gy = sobel_gradients(p)
        M[2:h, 2:w] = gx * gx + gy * gy
        horizontal[1:h - 1, 1:w - 1] = np.abs(gx) >= np.abs(gy)
    m = M[1:h + 1, 1:w + 1]
    before = np.where(horizontal, M[1:h + 1, 0:w], M[0:h, 1:w + 1])
    after = np.where(horizontal, M[1:h + 1, 2:w + 2], M[2:h + 2, 1:w + 1])
    return (m >= tau) & (m > before) & (m >= after)


def _contour_distances(S, T, R):
    """Row of the table: the R^2 + 2 counts of the pixels of S by the exact squared distance to the nearest pixel of T."""
    row = np.zeros(R * R + 2, dtype=np.uint64)
    ys, xs = np.nonzero(S)
    if len(ys) == 0:
        return row
    if not T.any():
        row[R * R + 1] = len(ys)
        return row
    iy, ix = ndimage.distance_transform_edt(~T, return_distances=False, return_indices=True)   # the nearest pixel of T, by index
    dy, dx = iy[ys, xs].astype(np.int64) - ys, ix[ys, xs].astype(np.int64) - xs
    d2 = dy * dy + dx * dx                                                                      # integers, never the float distance
    row[:] = np.bincount(np.where(d2 <= R * R, d2, R * R + 1), minlength=R * R + 2).astype(np.uint64)
    return row


def contour_statistics(a, b, regions, threshold, radius, planes=False):
    """What musica_sim_contours returns for every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side b): a
    list of dicts. The region's sub-array is its own domain: nothing outside it is read. E_a and E_b are contour_mask of the two
    sub-arrays at `threshold` tau, 1 .. 1 300 500 (processing.contour_threshold). For a source set S and a target set T every pixel
    s of S gets d^2(s) = the minimum over t in T of dx^2 + dy^2; its bin is d^2 where d^2 <= R^2 and R^2 + 1 ("far") otherwise, R the
    `radius`, 1 .. 32 (processing.contour_radius); an empty T puts every pixel of S into "far". "table": the (2, R^2 + 2) uint64 array
    of the bins' counts, direction 0 with S = E_a, T = E_b (where a's contours lie with respect to b's), direction 1 with S = E_b,
    T = E_a; a bin whose index is no sum of two squares stays 0. "contour_a", "contour_b": |E_a|, |E_b|. "pixels": w * h. With
    planes=True "planes": the (h, w) uint8 plane with bit 0 = E_a and bit 1 = E_b.
    Identities: row 0 sums to contour_a and row 1 to contour_b; table[0][0] == table[1][0] == |E_a and E_b|; swapping the sides swaps
    the rows; identical sides put everything into bin 0; the table at R' < R is the table at R with the bins R'^2 + 1 .. R^2 + 1
    folded into its far bin; complementing either side (255 - v) changes nothing; the same content at another origin gives the same
    table. The distances come from scipy's exact Euclidean distance transform, taken by the INDEX of the nearest target pixel and
    squared as integers."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("contour_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    tau, R = mp.contour_threshold(threshold), mp.contour_radius(radius)
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        Ea, Eb = contour_mask(a[ay:ay + h, ax:ax + w], tau), contour_mask(b[by:by + h, bx:bx + w], tau)
        d = {"table": np.stack([_contour_distances(Ea, Eb, R), _contour_distances(Eb, Ea, R)]), "contour_a": int(Ea.sum()), "contour_b": int(Eb.sum()),
             "pixels": w * h}
        if planes:
            d["planes"] = (Ea.astype(np.uint8) | (Eb.astype(np.uint8) << 1))
        res.append(d)
    return res


def _contour_quantile(counts, d2s, total, q):
    """The distance d of the ceil(q * total)-th found pixel in ascending order of d (total >= 1): the lower empirical quantile."""
    want = max(1, math.ceil(q * total - 1e-12))
    seen = 0
    for n, d2 in zip(counts, d2s):
        seen += n
        if seen >= want:
            return math.sqrt(d2)
    return math.sqrt(d2s[-1])


def contour_summary(table, radius, pixels):
    """What the study reports of a comparison's contours, in f64 from contour_statistics' (or musica_sim_contours') exact integers of ONE
    region only: one function for every study path. Row 0 of the table is a's contour pixels by their distance to b's, row 1 b's by
    their distance to a's (b the reference); "found" are the pixels of a row in the bins d^2 <= R^2. A dict:
        "contour_a", "contour_b"   the rows' sums; "density_a", "density_b": over the pixels; "ratio": contour_a / contour_b, None
                                   where b has no contour
        "fom"        Pratt's figure of merit: the sum over row 0's found pixels of 1 / (1 + d^2 / 9), divided by
                     max(contour_a, contour_b); None without contours
        "kept", "moved", "lost"    the shares of row 1 with d^2 <= 2, with 2 < d^2 <= R^2 and far; None where b has no contour
        "spurious"   row 0's far share; None where a has no contour
        "a_to_b", "b_to_a"         per direction "found", "far" and the "mean", "median" (the lower one) and "p95" of d over the found
                                   pixels, None without any
        "hausdorff"  the largest found d over both directions; None where any pixel is far or nothing was found."""
    R = mp.contour_radius(radius)
    t = np.asarray(table)
    if t.shape != (2, R * R + 2) or t.dtype.kind not in "iu":
        raise ValueError("the contour table of radius %d is (2, %d) integers, got %r %s" % (R, R * R + 2, t.shape, t.dtype))
    pixels = int(pixels)
    if pixels < 1:
        raise ValueError("a contour comparison has at least one pixel, got %d" % pixels)
    rows = [[int(v) for v in t[d]] for d in range(2)]
    na, nb = sum(rows[0]), sum(rows[1])
    out = {"contour_a": na, "contour_b": nb, "density_a": na / pixels, "density_b": nb / pixels, "ratio": na / nb if nb else None}
    out["fom"] = math.fsum(n / (1.0 + d2 / CONTOUR_FOM_SCALE) for d2, n in enumerate(rows[0][:R * R + 1]) if n) / max(na, nb) if max(na, nb) else None
    near = sum(rows[1][:min(CONTOUR_KEPT_D2, R * R) + 1])   # at R = 1 bin 2 is the far one: a diagonal neighbour is not resolved
    far_b, far_a = rows[1][R * R + 1], rows[0][R * R + 1]
    out["kept"] = near / nb if nb else None
    out["moved"] = (nb - near - far_b) / nb if nb else None
    out["lost"] = far_b / nb if nb else None
    out["spurious"] = far_a / na if na else None
    largest = None
    for name, row in zip(CONTOUR_DIRECTIONS, rows):
        hit = [(d2, n) for d2, n in enumerate(row[:R * R + 1]) if n]
        found = sum(n for _, n in hit)
        s = {"found": found, "far": row[R * R + 1], "mean": None, "median": None, "p95": None}
        if found:
            d2s, counts = [d2 for d2, _ in hit], [n for _, n in hit]
            s["mean"] = math.fsum(n * math.sqrt(d2) for d2, n in hit) / found
            s["median"] = _contour_quantile(counts, d2s, found, 0.5)
            s["p95"] = _contour_quantile(counts, d2s, found, 0.95)
            largest = max(largest or 0.0, math.sqrt(d2s[-1]))
        out[name] = s
    out["hausdorff"] = largest if (far_a == 0 and far_b == 0) else None
    return out


def contour_row(stats, threshold, radius):
    """A row's *_contours value from ONE dict of contour_statistics (or sim_contours): contour_summary's dict, "threshold", "radius",
    "pixels" and the exact "table" as nested lists; "planes" where the dict has them."""
    row = dict(contour_summary(stats["table"], radius, stats["pixels"]), threshold=mp.contour_threshold(threshold), radius=mp.contour_radius(radius),
               pixels=int(stats["pixels"]), table=np.asarray(stats["table"]).astype(np.uint64).tolist())
    if "planes" in stats:
        row["planes"] = np.asarray(stats["planes"], dtype=np.uint8)
    return row


# ---- the shape of a comparison: the Minkowski functionals of the level sets ----------------------------------------------------------------
# What does the gray-level landscape of the output look like as a shape: did the processing break one bright structure into islands, punch
# holes into solid ones, lengthen the iso-contours? The three Minkowski functionals of every threshold set {v >= t}, area, perimeter and
# Euler characteristic (components minus holes), are by Hadwiger's theorem all there is of additive, motion-invariant, continuous measures
# of a planar set. They are exact in integers and for all thresholds at once: on the closed cubical complex a cell (pixel, pixel edge,
# pixel corner) belongs to the set at t iff the MAXIMUM of its incident pixels is >= t, on the open complex iff their MINIMUM is, so eight
# 256-bin histograms of cell values a side give every curve and V - E + F the Euler characteristics: no labelling, no float.
# minkowski_statistics is the contract of musica_sim_minkowski (include/musica.h), whose tables are bit-identical to it;
# minkowski_summary is what the study reports of the integers, one function for every path.

MINKOWSKI_SIDES = ("a", "b", "min")    # the table's sides: the output, the reference, their pixel-wise minimum (the intersections of the upper sets)
MINKOWSKI_KINDS = ("face", "any_h", "any_v", "any_x", "all_h", "all_v", "all_x", "outline")   # the table's rows
MINKOWSKI_CURVES = ("area", "perimeter", "euler8", "euler4", "contact")                      # minkowski_curves' rows
MINKOWSKI_FRACTIONS = 7                # the matched read-out: the area fractions k / 8, k = 1 .. 7
MINKOWSKI_SIDE_KEYS = ("mean", "tv", "islands", "islands_level", "holes", "holes_level", "contact")   # each with _a and _b
MINKOWSKI_KEYS = tuple("%s_%s" % (k, s) for s in "ab" for k in MINKOWSKI_SIDE_KEYS) + \
    ("tv_gain", "area_l1", "perimeter_l1", "euler8_l1", "euler4_l1", "overlap", "overlap_min", "overlap_min_level", "matched_perimeter_l1", "matched_euler8_l1")
MINKOWSKI_MATCHED_KEYS = ("fraction", "level_a", "level_b", "perimeter_a", "perimeter_b", "euler8_a", "euler8_b", "euler4_a", "euler4_b")


def minkowski_cells(p):
    """The eight cell-value histograms of ONE 2-D uint8 plane, which is its own domain: the (8, 256) uint32 array [kind][value] of
    MINKOWSKI_KINDS. A pixel that does not exist takes no part in a maximum (any_*); a cell that would need one is no cell of all_*."""
    p = np.asarray(p, dtype=np.uint8)
    z = np.pad(p, 1)   # a frame of zeros: the maximum over the pixels that exist
    cells = (p,
             np.maximum(z[1:-1, :-1], z[1:-1, 1:]),                                                    # h x (w + 1)
             np.maximum(z[:-1, 1:-1], z[1:, 1:-1]),                                                    # (h + 1) x w
             np.maximum(np.maximum(z[:-1, :-1], z[:-1, 1:]), np.maximum(z[1:, :-1], z[1:, 1:])),      # (h + 1) x (w + 1)
             np.minimum(p[:, :-1], p[:, 1:]),                                                          # h x (w - 1)
             np.minimum(p[:-1, :], p[1:, :]),                                                          # (h - 1) x w
             np.minimum(np.minimum(p[:-1, :-1], p[:-1, 1:]), np.minimum(p[1:, :-1], p[1:, 1:])),      # (h - 1) x (w - 1)
             np.concatenate([p[0, :], p[-1, :], p[:, 0], p[:, -1]]))                                   # 2 w + 2 h
    return np.stack([np.bincount(c.ravel(), minlength=256) for c in cells]).astype(np.uint32)


def minkowski_statistics(a, b, regions):
    """What musica_sim_minkowski returns for every region (ax, ay, bx, by, w, h), w, h >= 1, of two 2-D uint8 planes (side a, side b): a
    list of dicts. The region's sub-array is its own domain: nothing outside it is read. "table": the (3, 8, 256) uint32 array
    [side a = 0, b = 1, min(a, b) = 2][kind][value] of minkowski_cells: the number of cells of a kind (MINKOWSKI_KINDS: the pixels; the
    pixel edges between horizontal and between vertical neighbours and the pixel corners by the maximum of their pixels that exist, the
    outline's included; the interior edges and corners by the minimum of theirs; the 2 w + 2 h outline edges by their one pixel) whose
    value is v. Nothing is cumulated. "pixels": w * h. Every row sums to its number of cells: w h, h (w + 1), (h + 1) w,
    (h + 1) (w + 1), h (w - 1), (h - 1) w, (h - 1) (w - 1), 2 w + 2 h."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("minkowski_statistics needs two 2-D uint8 planes, got %r %s and %r %s" % (a.shape, a.dtype, b.shape, b.dtype))
    res = []
    for region in regions:
        ax, ay, bx, by, w, h = (int(v) for v in region)
        if min(ax, ay, bx, by) < 0 or w < 1 or h < 1 or ax + w > a.shape[1] or ay + h > a.shape[0] or bx + w > b.shape[1] or by + h > b.shape[0]:
            raise ValueError("region %r is empty or leaves the %r / %r planes" % (tuple(region), a.shape, b.shape))
        sa, sb = a[ay:ay + h, ax:ax + w], b[by:by + h, bx:bx + w]
        res.append({"table": np.stack([minkowski_cells(sa), minkowski_cells(sb), minkowski_cells(np.minimum(sa, sb))]), "pixels": w * h})
    return res


def minkowski_curves(table):
    """The Minkowski functionals of the threshold sets {v >= t}, t = 0 .. 255, from a (3, 8, 256) table of minkowski_statistics: the
    (3, 5, 256) int64 array [side][MINKOWSKI_CURVES][t]. With N_k(t) the cells of kind k whose value is at least t: area = N0;
    perimeter = N1 + N2 - N7 - N4 - N5, the interior pixel edges with exactly one side in the set (the region's outline is not charged);
    euler8 = N3 - N1 - N2 + N0, the 8-connected components minus the 4-connected holes (the closed complex); euler4 = N0 - N4 - N5 + N6,
    the 4-connected components minus the 8-connected holes (the open complex); contact = N7, the outline edges that the set touches."""
    t = np.asarray(table)
    if t.shape != (len(MINKOWSKI_SIDES), len(MINKOWSKI_KINDS), 256) or t.dtype.kind not in "iu":
        raise ValueError("a Minkowski table is (3, 8, 256) integers, got %r %s" % (t.shape, t.dtype))
    N = np.cumsum(t.astype(np.int64)[:, :, ::-1], axis=2)[:, :, ::-1]
    return np.stack([N[:, 0], N[:, 1] + N[:, 2] - N[:, 7] - N[:, 4] - N[:, 5], N[:, 3] - N[:, 1] - N[:, 2] + N[:, 0],
                     N[:, 0] - N[:, 4] - N[:, 5] + N[:, 6], N[:, 7]], axis=1)


def _minkowski_l1(fa, fb):
    """sum |fa - fb| / sum (|fa| + |fb|) of two lists of integers, None where the denominator is 0."""
    den = sum(abs(x) + abs(y) for x, y in zip(fa, fb))
    return sum(abs(x - y) for x, y in zip(fa, fb)) / den if den else None


def minkowski_summary(table, pixels):
    """What the study reports of a comparison's level sets, in f64 from minkowski_statistics' (or musica_sim_minkowski's) exact integers
    of ONE region only: one function for every study path. All sums run over the levels t = 1 .. 255; a quotient whose denominator is 0
    is None. A dict: "pixels"; per side s in a, b "mean_s" = sum area / pixels (the mean gray level), "tv_s" = sum perimeter / pixels
    (the anisotropic total variation a pixel, by the co-area formula), "islands_s" the maximum of euler8 and "islands_level_s" the lowest
    level that reaches it, "holes_s" minus the minimum of euler8, floored at 0, and "holes_level_s" the lowest level of that minimum,
    "contact_s" = sum contact / (255 * the outline's edges); "tv_gain" = tv_a / tv_b; "area_l1", "perimeter_l1", "euler8_l1",
    "euler4_l1" = sum |f_a - f_b| / sum (|f_a| + |f_b|); "overlap" = sum area_min / sum (area_a + area_b - area_min), the Ruzicka
    similarity sum min / sum max; "overlap_min" the smallest Jaccard index of a level whose union is not empty, "overlap_min_level" the
    lowest such level; "matched", the tone-free read-out: for k = 1 .. 7 a dict of "fraction" k / 8, "level_a" and "level_b", on either
    side the largest t in 0 .. 255 with 8 area(t) >= k pixels, and "perimeter", "euler8" and "euler4" of either side at its own level;
    "matched_perimeter_l1" and "matched_euler8_l1", the same normalised L1 over the seven. Where a is a strictly increasing function of
    b the two sides have the same family of upper sets, so the seven pairs are equal and the two distances 0.0."""
    c = minkowski_curves(table)
    pixels = int(pixels)
    if pixels < 1 or int(c[0, 0, 0]) != pixels:
        raise ValueError("the Minkowski table holds %d pixels, got pixels = %d" % (int(c[0, 0, 0]), pixels))
    area, perimeter, euler8, euler4, contact = ([[int(v) for v in c[s, k]] for s in range(3)] for k in range(len(MINKOWSKI_CURVES)))
    outline = int(c[0, 4, 0])   # 2 w + 2 h
    out = {"pixels": pixels}
    for s, name in enumerate("ab"):
        e = euler8[s][1:]
        top, low = max(e), min(e)
        out.update({"mean_" + name: sum(area[s][1:]) / pixels, "tv_" + name: sum(perimeter[s][1:]) / pixels,
                    "islands_" + name: top, "islands_level_" + name: 1 + e.index(top),
                    "holes_" + name: max(0, -low), "holes_level_" + name: 1 + e.index(low),
                    "contact_" + name: sum(contact[s][1:]) / (255 * outline)})
    out = {k: out[k] for k in ("pixels",) + MINKOWSKI_KEYS[:2 * len(MINKOWSKI_SIDE_KEYS)]}
    out["tv_gain"] = out["tv_a"] / out["tv_b"] if out["tv_b"] else None
    for k, f in (("area", area), ("perimeter", perimeter), ("euler8", euler8), ("euler4", euler4)):
        out[k + "_l1"] = _minkowski_l1(f[0][1:], f[1][1:])
    union = [x + y - z for x, y, z in zip(area[0], area[1], area[2])]
    out["overlap"] = sum(area[2][1:]) / sum(union[1:]) if sum(union[1:]) else None
    out["overlap_min"], out["overlap_min_level"] = None, None
    for t in range(1, 256):
        if union[t] and (out["overlap_min"] is None or area[2][t] / union[t] < out["overlap_min"]):
            out["overlap_min"], out["overlap_min_level"] = area[2][t] / union[t], t
    matched = []
    for k in range(1, MINKOWSKI_FRACTIONS + 1):
        ta, tb = (max(t for t in range(256) if 8 * area[s][t] >= k * pixels) for s in range(2))   # t = 0 always qualifies
        matched.append({"fraction": k / 8, "level_a": ta, "level_b": tb, "perimeter_a": perimeter[0][ta], "perimeter_b": perimeter[1][tb],
                        "euler8_a": euler8[0][ta], "euler8_b": euler8[1][tb], "euler4_a": euler4[0][ta], "euler4_b": euler4[1][tb]})
    out["matched_perimeter_l1"] = _minkowski_l1([m["perimeter_a"] for m in matched], [m["perimeter_b"] for m in matched])
    out["matched_euler8_l1"] = _minkowski_l1([m["euler8_a"] for m in matched], [m["euler8_b"] for m in matched])
    out["matched"] = matched
    return out


def minkowski_row(stats, curves=False):
    """A row's *_minkowski value from ONE dict of minkowski_statistics (or sim_minkowski): minkowski_summary's dict and the exact
    "table" as nested lists; with curves=True also "curves", minkowski_curves' (3, 5, 256) int64 array."""
    row = dict(minkowski_summary(stats["table"], stats["pixels"]), table=np.asarray(stats["table"]).astype(np.uint32).tolist())
    if curves:
        row["curves"] = minkowski_curves(stats["table"])
    return row

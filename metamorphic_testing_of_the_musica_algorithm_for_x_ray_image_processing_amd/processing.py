"""ctypes mirror of the reference's pipeline object on top of libmusica_hip.so.

`MusicaProcessing` keeps the public surface of `class VulkanProcessing`
(reference include/vk_processing.h:281-355): init(imageSize), execute(imageData),
saveOutImage(filePath), debugProcess(), cleanup(), getImageSize() — same argument
meaning, `bool` results, and an error line on stderr when a call fails. Everything
else (`batch`, `levels`, getters for intermediates) is the extension surface the
parity tests and the batch driver use.

There is no CPU fallback: the shared library is HIP-only and every call fails
loudly when the extension or a GPU is missing.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmusica_hip.so")
CLI_PATH = os.path.join(_HERE, "musica-standalone")

MAX_POINTS = 256
NOISE_BINS = 2048
GRAD_BINS = 1024
OUT_MARGIN = 10

HIST_RENDER_WIDTH, HIST_RENDER_HEIGHT = 512, 128   # histRenderWidth / histRenderHeight, include/vk_processing.h:31-32

FLAG_CLAHE = 0x1
FLAG_NO_GRAPH = 0x2
FLAG_GENERIC_KERNELS = 0x4
FLAG_NO_AUTOTUNE = 0x8
FLAG_LINEAR = 0x10
FLAG_REFERENCE_ORDER = 0x20
FLAG_ONE_SHOT = 0x40

IMG_NORMALIZED, IMG_DOWNSAMPLED, IMG_BANDPASS, IMG_SDEV, IMG_CNR, IMG_EXPAND = 0, 1, 2, 3, 4, 5
IMG_GRADED, IMG_RELEVANT, IMG_LOWPASS, IMG_EXP_BANDPASS, IMG_SQRT, IMG_CLAHE_GRADED, IMG_CONTRAST_BAND = 6, 7, 8, 9, 10, 11, 12
STAGE_NORM, STAGE_REDUCE, STAGE_ANALYSIS, STAGE_EXPAND, STAGE_GRADATION = 0, 1, 2, 3, 4

KERNEL_NAMES = ["minmax", "normalize", "reduce_l0", "reduce_rest", "band_l0", "band_rest", "sdev_hist", "curves",
                "cnr", "expand_l0", "expand_rest", "grad_hist", "grad_curve", "grad_apply"]
KERNEL_ID = {n: i for i, n in enumerate(KERNEL_NAMES)}


class Params(C.Structure):
    _fields_ = [("image_size", C.c_uint32), ("levels", C.c_uint32), ("batch", C.c_uint32),
                ("device", C.c_int32), ("flags", C.c_uint32)]


class Tunables(C.Structure):
    """musica_tunables (include/musica.h): the constants of include/vk_processing.h:39-49 and the two LINEAR_* #defines of :16-17."""
    _fields_ = [("nr_high_cnr", C.c_float), ("nr_max_high_factor", C.c_float), ("nr_low_cnr", C.c_float), ("nr_min_low_factor", C.c_float),
                ("high_contrast_max_reduction", C.c_float), ("low_contrast_max_enhancement", C.c_float),
                ("linear_low_contrast", C.c_uint32), ("linear_high_contrast", C.c_uint32)]


def default_tunables(**overrides):
    """The reference's values, with keyword overrides (e.g. linear_low_contrast=1, nr_low_cnr=2.5)."""
    t = Tunables()
    load_library().musica_tunables_default(C.byref(t))
    for k, v in overrides.items():
        if k not in dict(Tunables._fields_):
            raise KeyError(k)
        setattr(t, k, v)
    return t


class HistMaxPoint(C.Structure):
    _fields_ = [("maxValue", C.c_uint32), ("maxBin", C.c_uint32)]


class ContrastParams(C.Structure):
    _fields_ = [("lowContrastFactor", C.c_float), ("highContrastFactor", C.c_float)]


class Point(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class ContrastCurve(C.Structure):
    _fields_ = [("points", Point * MAX_POINTS), ("pointsCount", C.c_uint32)]

    def as_array(self):
        return np.array([(self.points[i].x, self.points[i].y) for i in range(self.pointsCount)], dtype=np.float32)


class NrParams(C.Structure):
    _fields_ = [("lowCnr", C.c_float), ("lowFactor", C.c_float), ("highCnr", C.c_float), ("highFactor", C.c_float)]


class GradCurve(C.Structure):
    _fields_ = [("points", Point * MAX_POINTS), ("pointsCount", C.c_uint32),
                ("t0", C.c_float), ("ta", C.c_float), ("t1", C.c_float)]

    def as_array(self):
        return np.array([(self.points[i].x, self.points[i].y) for i in range(self.pointsCount)], dtype=np.float32)


class Stats(C.Structure):
    _fields_ = [("image_id", C.c_uint32), ("min_sqrt", C.c_float), ("max_sqrt", C.c_float),
                ("noise_max_bin", C.c_uint32 * 4), ("noise_max_value", C.c_uint32 * 4),
                ("grad_max_bin", C.c_uint32), ("grad_max_value", C.c_uint32),
                ("mean_cnr", C.c_float), ("t0", C.c_float), ("ta", C.c_float), ("t1", C.c_float)]

    FLOAT_FIELDS = ("min_sqrt", "max_sqrt", "mean_cnr", "t0", "ta", "t1")

    def as_row(self):
        """The struct as a flat list of 14 floats (comparisons in tests; the gather itself moves the raw bytes)."""
        return [float(self.image_id), self.min_sqrt, self.max_sqrt] + [float(v) for v in self.noise_max_bin] + \
               [float(self.grad_max_bin), self.mean_cnr, self.t0, self.ta, self.t1, float(self.grad_max_value)]


SIM_SLOTS = 8               # MUSICA_SIM_SLOTS
SIM_MAX_QUERIES = 64        # MUSICA_SIM_MAX_QUERIES
SIM_METRICS = ("mse", "ssim", "hist_intersection", "hist_distance", "hist_bhattacharyya")   # harness.similarities' keys


class SimQuery(C.Structure):
    """musica_sim_query: image `image_index`'s output at (ax, ay) against reference slot `slot` at (bx, by), w x h output pixels."""
    _fields_ = [(n, C.c_uint32) for n in ("image_index", "slot", "ax", "ay", "bx", "by", "w", "h")]


class SimResult(C.Structure):
    _fields_ = [(n, C.c_double) for n in SIM_METRICS] + \
               [("sq_diff_sum", C.c_uint64), ("pixels", C.c_uint64), ("bins_a", C.c_uint32 * 256), ("bins_b", C.c_uint32 * 256),
                ("min_a", C.c_uint32), ("max_a", C.c_uint32), ("min_b", C.c_uint32), ("max_b", C.c_uint32)]

    def as_dict(self):
        d = {n: getattr(self, n) for n in SIM_METRICS}
        d.update(sq_diff_sum=int(self.sq_diff_sum), pixels=int(self.pixels),
                 bins_a=np.ctypeslib.as_array(self.bins_a).astype(np.int64), bins_b=np.ctypeslib.as_array(self.bins_b).astype(np.int64),
                 min_a=int(self.min_a), max_a=int(self.max_a), min_b=int(self.min_b), max_b=int(self.max_b))
        return d


JOINT_METRICS = ("mi", "nmi", "corr_ratio", "tone_mse", "tone_ssim")   # harness.tone_similarities' keys (tone_ssim: not in SimJointResult)


class SimJointResult(C.Structure):
    """musica_sim_joint_result: the tone metrics of one comparison, from its exact joint histogram."""
    _fields_ = [(n, C.c_double) for n in ("mi", "nmi", "corr_ratio", "tone_mse", "h_a", "h_b", "h_ab")] + \
               [("pixels", C.c_uint64), ("sq_diff_sum", C.c_uint64), ("tone_lut", C.c_uint8 * 256)]

    def as_dict(self):
        d = {n: getattr(self, n) for n in ("mi", "nmi", "corr_ratio", "tone_mse", "h_a", "h_b", "h_ab")}
        d.update(pixels=int(self.pixels), sq_diff_sum=int(self.sq_diff_sum), tone_lut=np.ctypeslib.as_array(self.tone_lut).copy())
        return d


SIM_MAX_RADIUS = 16         # MUSICA_SIM_MAX_RADIUS
BLUR_MAX_RADIUS = 8         # MUSICA_BLUR_MAX_RADIUS
ZOOM_MAX_P = 32             # MUSICA_ZOOM_MAX_P
SCATTER_MAX_RADIUS = 127    # MUSICA_SCATTER_MAX_RADIUS
SCATTER_MAX_DEN = 64        # MUSICA_SCATTER_MAX_DEN
WARP_GRID = 64              # MUSICA_WARP_GRID
WARP_UNIT = 256             # MUSICA_WARP_UNIT
WARP_MAX_SHIFT = 4096       # MUSICA_WARP_MAX_SHIFT
WARP_MAX_NODES = 258        # MUSICA_WARP_MAX_NODES
SIM_TILE = 64               # MUSICA_SIM_TILE
DETAIL_MAX_RADIUS = 64      # MUSICA_DETAIL_MAX_RADIUS
DETAIL_MAX_CONTRAST = 512   # MUSICA_DETAIL_MAX_CONTRAST
DETAIL_MAX = 1024           # MUSICA_DETAIL_MAX
EDGE_MIN_HALF = 8           # MUSICA_EDGE_MIN_HALF
EDGE_MAX_HALF = 128         # MUSICA_EDGE_MAX_HALF
EDGE_MIN_Q = 4              # MUSICA_EDGE_MIN_Q
EDGE_MAX_Q = 16             # MUSICA_EDGE_MAX_Q
EDGE_MAX_CONTRAST = 512     # MUSICA_EDGE_MAX_CONTRAST
EDGE_MAX = 256              # MUSICA_EDGE_MAX
EDGE_BINS_MAX = 2048        # MUSICA_EDGE_BINS_MAX
GRATING_MIN_HALF = 8        # MUSICA_GRATING_MIN_HALF
GRATING_MAX_HALF = 128      # MUSICA_GRATING_MAX_HALF
GRATING_MAX_U = 8           # MUSICA_GRATING_MAX_U
GRATING_MAX_PERIOD = 64     # MUSICA_GRATING_MAX_PERIOD
GRATING_MAX_CONTRAST = 512  # MUSICA_GRATING_MAX_CONTRAST
GRATING_MAX = 256           # MUSICA_GRATING_MAX
POINT_MIN_RADIUS = 4        # MUSICA_POINT_MIN_RADIUS
POINT_MAX_RADIUS = 32       # MUSICA_POINT_MAX_RADIUS
POINT_MAX_SIZE = 3          # MUSICA_POINT_MAX_SIZE
POINT_MIN_CONTRAST = -64512  # MUSICA_POINT_MIN_CONTRAST
POINT_MAX_CONTRAST = 1024   # MUSICA_POINT_MAX_CONTRAST
POINT_MAX_GROUPS = 16       # MUSICA_POINT_MAX_GROUPS
POINT_MAX = 4096            # MUSICA_POINT_MAX
GAIN_ONE = 4096             # MUSICA_GAIN_ONE
PROFILE_MAX_QUERIES = 16    # MUSICA_PROFILE_MAX_QUERIES
LUT_ENTRIES = 65536         # MUSICA_LUT_ENTRIES
LEVEL_MAX_QUERIES = 4       # MUSICA_LEVEL_MAX_QUERIES
LEVEL_MIN_SHIFT = 4         # MUSICA_LEVEL_MIN_SHIFT
LEVEL_MAX_SHIFT = 15        # MUSICA_LEVEL_MAX_SHIFT
GRADIENT_CLASSES = 22       # MUSICA_GRADIENT_CLASSES: the bit lengths of B <= 1 300 500
GRADIENT_C = 2720           # MUSICA_GRADIENT_C
ORDER_RINGS = 3             # MUSICA_ORDER_RINGS: max(|dx|, |dy|) = 1, 2, 3 with 8, 16 and 24 neighbours
ORDER_BINS = 97             # MUSICA_ORDER_BINS: the census distance d = 0 .. 96
REACH_MAX_RADII = 32        # MUSICA_REACH_MAX_RADII
REACH_MAX_RADIUS = 16383    # MUSICA_REACH_MAX_RADIUS
REACH_MAX_QUERIES = 16      # MUSICA_REACH_MAX_QUERIES
OBSERVER_MAX_VIEWS = 1024   # MUSICA_OBSERVER_MAX_VIEWS
OBSERVER_MAX_BANKS = 8      # MUSICA_OBSERVER_MAX_BANKS
OBSERVER_MAX_CHANNELS = 16  # MUSICA_OBSERVER_MAX_CHANNELS
OBSERVER_MAX_HALF = 66      # MUSICA_OBSERVER_MAX_HALF: 2 * 32 + 2, the box of a radius-32 detail
LATTICE_MAX_PERIOD = 32     # MUSICA_LATTICE_MAX_PERIOD
LATTICE_MAX_QUERIES = 16    # MUSICA_LATTICE_MAX_QUERIES
BLOBS_MAX_QUERIES = 4       # MUSICA_BLOBS_MAX_QUERIES
BLOB_CLASSES = 32           # MUSICA_BLOB_CLASSES
SPECTRUM_MAX_TILE = 64      # MUSICA_SPECTRUM_MAX_TILE
SPECTRUM_MAX_QUERIES = 4    # MUSICA_SPECTRUM_MAX_QUERIES
SPECTRUM_TILES = (8, 16, 32, 64)
COOCCURRENCE_MAX_DISTANCES = 4   # MUSICA_COOCCURRENCE_MAX_DISTANCES
COOCCURRENCE_MAX_DISTANCE = 16   # MUSICA_COOCCURRENCE_MAX_DISTANCE
COOCCURRENCE_MAX_LEVELS = 64     # MUSICA_COOCCURRENCE_MAX_LEVELS
COOCCURRENCE_MAX_QUERIES = 4     # MUSICA_COOCCURRENCE_MAX_QUERIES
COOCCURRENCE_LEVELS = (8, 16, 32, 64)
COOCCURRENCE_DISTANCES = (1, 2, 4, 8)   # the study's default distance list
GRANULOMETRY_MAX_RADII = 8       # MUSICA_GRANULOMETRY_MAX_RADII
GRANULOMETRY_MAX_RADIUS = 16     # MUSICA_GRANULOMETRY_MAX_RADIUS
GRANULOMETRY_MAX_QUERIES = 4     # MUSICA_GRANULOMETRY_MAX_QUERIES
GRANULOMETRY_WORDS = 5           # MUSICA_GRANULOMETRY_WORDS
GRANULOMETRY_RADII = (1, 2, 4, 8, 16)   # the study's default radii list
CONTOURS_MAX_RADIUS = 32         # MUSICA_CONTOURS_MAX_RADIUS
CONTOURS_MAX_QUERIES = 4         # MUSICA_CONTOURS_MAX_QUERIES
CONTOURS_MAX_THRESHOLD = 1300500 # MUSICA_CONTOURS_MAX_THRESHOLD: 1020^2 + 510^2, the largest squared Sobel gradient of a uint8 plane
CONTOURS_THRESHOLD = 4096        # the command line's default: |g| >= 64, a straight step of 16 of 255 gray levels
CONTOURS_RADIUS = 16             # the study's default radius
MINKOWSKI_MAX_QUERIES = 4        # MUSICA_MINKOWSKI_MAX_QUERIES
MINKOWSKI_KINDS = 8              # MUSICA_MINKOWSKI_KINDS: face, any_h, any_v, any_x, all_h, all_v, all_x, outline
MINKOWSKI_SIDES = 3              # MUSICA_MINKOWSKI_SIDES: a, b, min(a, b)


def zoom_ratio(zoom):
    """(p, q) of a magnification p / q as harness.zoom and the library take it: integers 1 <= q < p <= ZOOM_MAX_P in lowest terms, else
    ValueError."""
    try:
        p, q = zoom
        if p != int(p) or q != int(q):
            raise TypeError
        p, q = int(p), int(q)
    except (TypeError, ValueError):
        raise ValueError("a zoom is a pair of integers (p, q), got %r" % (zoom,))
    if not 1 <= q < p <= ZOOM_MAX_P:
        raise ValueError("zoom %d / %d is not 1 <= q < p <= %d" % (p, q, ZOOM_MAX_P))
    if math.gcd(p, q) != 1:
        raise ValueError("zoom %d / %d is not in lowest terms" % (p, q))
    return p, q


def codec_table_words(table):
    """A quantiser table as metrics.block_codec and the library take it: 8 x 8 integers 1 .. 65535, indexed [v][u], as a C-contiguous
    (8, 8) uint16 array; else ValueError."""
    try:
        t = np.asarray(table)
        if t.shape != (8, 8) or t.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("a codec table is 8 x 8 integers, got %r" % (table,))
    if int(t.min()) < 1 or int(t.max()) > 65535:
        raise ValueError("codec table entries are 1 .. 65535, got %d .. %d" % (int(t.min()), int(t.max())))
    return np.ascontiguousarray(t, dtype=np.uint16)


def lattice_period(period, origin):
    """(P, o) of a lattice as metrics.lattice_statistics and the library take it: P one of 2, 4, 8, 16, 32 and the origin 0 <= o < P,
    integers, else ValueError."""
    try:
        if period != int(period) or origin != int(origin):
            raise TypeError
        P, o = int(period), int(origin)
    except (TypeError, ValueError):
        raise ValueError("a lattice is a period and an origin, integers, got %r, %r" % (period, origin))
    if P not in (2, 4, 8, 16, 32):
        raise ValueError("lattice period %d is not one of 2, 4, 8, 16, 32" % P)
    if not 0 <= o < P:
        raise ValueError("lattice origin %d is not in 0 .. %d" % (o, P - 1))
    return P, o


def spectrum_tile(tile):
    """The tile side T of a Walsh spectrum as metrics.spectrum_statistics and the library take it: one of 8, 16, 32, 64, an integer, else
    ValueError."""
    try:
        if isinstance(tile, (bool, np.bool_, str)) or tile != int(tile):
            raise TypeError
        T = int(tile)
    except (TypeError, ValueError):
        raise ValueError("a spectrum tile is one of 8, 16, 32, 64, got %r" % (tile,))
    if T not in SPECTRUM_TILES:
        raise ValueError("spectrum tile %d is not one of 8, 16, 32, 64" % T)
    return T


def cooccurrence_levels(levels):
    """The gray levels G of a co-occurrence table as metrics.cooccurrence_statistics and the library take them: one of 8, 16, 32, 64, an
    integer, else ValueError."""
    try:
        if isinstance(levels, (bool, np.bool_, str)) or levels != int(levels):
            raise TypeError
        G = int(levels)
    except (TypeError, ValueError):
        raise ValueError("co-occurrence levels are one of 8, 16, 32, 64, got %r" % (levels,))
    if G not in COOCCURRENCE_LEVELS:
        raise ValueError("co-occurrence levels %d are not one of 8, 16, 32, 64" % G)
    return G


def cooccurrence_distances(distances):
    """The distance list of a co-occurrence table as metrics.cooccurrence_statistics and the library take it: a tuple of 1 ..
    COOCCURRENCE_MAX_DISTANCES distinct ascending integers, each 1 .. COOCCURRENCE_MAX_DISTANCE, else ValueError."""
    try:
        if isinstance(distances, (str, bytes)):
            raise TypeError
        given = list(distances)
        if any(isinstance(d, (bool, np.bool_, str)) or d != int(d) for d in given):
            raise TypeError
        ds = tuple(int(d) for d in given)
    except (TypeError, ValueError):
        raise ValueError("co-occurrence distances are a list of integers, got %r" % (distances,))
    if not 1 <= len(ds) <= COOCCURRENCE_MAX_DISTANCES:
        raise ValueError("co-occurrence takes 1 .. %d distances, got %d" % (COOCCURRENCE_MAX_DISTANCES, len(ds)))
    for d in ds:
        if not 1 <= d <= COOCCURRENCE_MAX_DISTANCE:
            raise ValueError("co-occurrence distance %d is not in 1 .. %d" % (d, COOCCURRENCE_MAX_DISTANCE))
    if any(y <= x for x, y in zip(ds, ds[1:])):
        raise ValueError("co-occurrence distances are distinct and ascending, got %r" % (ds,))
    return ds


def granulometry_radii(radii):
    """The radii list of a granulometry as metrics.granulometry_statistics and the library take it: a tuple of 1 ..
    GRANULOMETRY_MAX_RADII distinct ascending integers, each 1 .. GRANULOMETRY_MAX_RADIUS, else ValueError."""
    try:
        if isinstance(radii, (str, bytes)):
            raise TypeError
        given = list(radii)
        if any(isinstance(r, (bool, np.bool_, str)) or r != int(r) for r in given):
            raise TypeError
        rs = tuple(int(r) for r in given)
    except (TypeError, ValueError):
        raise ValueError("granulometry radii are a list of integers, got %r" % (radii,))
    if not 1 <= len(rs) <= GRANULOMETRY_MAX_RADII:
        raise ValueError("granulometry takes 1 .. %d radii, got %d" % (GRANULOMETRY_MAX_RADII, len(rs)))
    for r in rs:
        if not 1 <= r <= GRANULOMETRY_MAX_RADIUS:
            raise ValueError("granulometry radius %d is not in 1 .. %d" % (r, GRANULOMETRY_MAX_RADIUS))
    if any(y <= x for x, y in zip(rs, rs[1:])):
        raise ValueError("granulometry radii are distinct and ascending, got %r" % (rs,))
    return rs


def _contour_integer(value, what, lo, hi):
    try:
        if isinstance(value, (bool, np.bool_, str, bytes, float, np.floating)) or value != int(value):
            raise TypeError
        v = int(value)
    except (TypeError, ValueError):
        raise ValueError("contours: %s is an integer %d .. %d, got %r" % (what, lo, hi, value))
    if not lo <= v <= hi:
        raise ValueError("contours: %s %d is not in %d .. %d" % (what, v, lo, hi))
    return v


def contour_threshold(threshold):
    """The threshold tau on the squared Sobel gradient gx^2 + gy^2 of a contour pixel, as metrics.contour_statistics and the library
    take it: an integer 1 .. CONTOURS_MAX_THRESHOLD, else ValueError (a bool, a float and a string are refused whatever they hold)."""
    return _contour_integer(threshold, "the threshold", 1, CONTOURS_MAX_THRESHOLD)


def contour_radius(radius):
    """The radius R up to which the distance between two contour sets is resolved, as metrics.contour_statistics and the library take
    it: an integer 1 .. CONTOURS_MAX_RADIUS, else ValueError (a bool, a float and a string are refused whatever they hold)."""
    return _contour_integer(radius, "the radius", 1, CONTOURS_MAX_RADIUS)


def blob_threshold(threshold):
    """The threshold t of a change mask |a - b| > t as metrics.blob_statistics and the library take it: an integer 0 .. 254, else
    ValueError."""
    try:
        if isinstance(threshold, (bool, np.bool_, str)) or threshold != int(threshold):
            raise TypeError
        t = int(threshold)
    except (TypeError, ValueError):
        raise ValueError("a blob threshold is an integer 0 .. 254, got %r" % (threshold,))
    if not 0 <= t <= 254:
        raise ValueError("blob threshold %d is not in 0 .. 254" % t)
    return t


def scatter_spec(spec):
    """(R, a, b) of a veil as harness.scatter and the library take it: the box radius 1 <= R <= SCATTER_MAX_RADIUS and the scatter
    fraction a / b, integers 1 <= a < b <= SCATTER_MAX_DEN in lowest terms, else ValueError."""
    try:
        r, a, b = spec
        if r != int(r) or a != int(a) or b != int(b):
            raise TypeError
        r, a, b = int(r), int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError("a scatter is a triple of integers (R, a, b), got %r" % (spec,))
    if not 1 <= r <= SCATTER_MAX_RADIUS:
        raise ValueError("scatter radius %d is not in 1 .. %d" % (r, SCATTER_MAX_RADIUS))
    if not 1 <= a < b <= SCATTER_MAX_DEN:
        raise ValueError("scatter fraction %d / %d is not 1 <= a < b <= %d" % (a, b, SCATTER_MAX_DEN))
    if math.gcd(a, b) != 1:
        raise ValueError("scatter fraction %d / %d is not in lowest terms" % (a, b))
    return r, a, b


def warp_nodes(n, origin=0):
    """How many nodes a side the field of a plane of side n at `origin` needs: ((n - 1 + origin) >> 6) + 2."""
    return ((int(n) - 1 + int(origin)) >> 6) + 2


def warp_field(field, n, origin=0):
    """A displacement field as harness.warp and the library take it for a plane of side n at `origin` (one integer for both axes): a
    contiguous int16 array (M, M, 2), field[j, i] = (dx, dy) of node (row j, column i) in units of 1 / WARP_UNIT pixel, else ValueError:
    an origin outside 0 .. WARP_GRID - 1, an array of integers that is not (M, M, 2), M below warp_nodes(n, origin) or above
    WARP_MAX_NODES, a component beyond +-WARP_MAX_SHIFT. The same check as the C side's."""
    if isinstance(origin, bool) or not isinstance(origin, (int, np.integer)) or not 0 <= origin < WARP_GRID:
        raise ValueError("origin %r is not an integer in 0 .. %d" % (origin, WARP_GRID - 1))
    a = np.asarray(field)
    if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 2 or a.dtype.kind not in "iu":
        raise ValueError("a field is an (M, M, 2) array of integers, got %r %s" % (a.shape, a.dtype))
    need = warp_nodes(n, origin)
    if a.shape[0] < need:
        raise ValueError("%d nodes a side are fewer than the %d that a plane of %d pixels at origin %d needs" % (a.shape[0], need, int(n), origin))
    if a.shape[0] > WARP_MAX_NODES:
        raise ValueError("%d nodes a side are more than %d" % (a.shape[0], WARP_MAX_NODES))
    if int(a.min()) < -WARP_MAX_SHIFT or int(a.max()) > WARP_MAX_SHIFT:
        j, i, k = (int(v[0]) for v in np.nonzero(abs(a.astype(np.int64)) > WARP_MAX_SHIFT))
        raise ValueError("node (row %d, column %d) has the component %d, beyond +-%d" % (j, i, int(a[j, i, k]), WARP_MAX_SHIFT))
    return np.ascontiguousarray(a, dtype=np.int16)


def _ints(t, k):
    """The k integers of an item as a tuple of ints; TypeError or ValueError otherwise."""
    t = tuple(t)
    out = tuple(map(int, t))
    if len(out) != k or out != t:   # elementwise ==: 3.0 is 3, 3.5 is not
        raise TypeError
    return out


def _patch_list(items, n, name, holds, most, parse, check, square):
    """What detail_list, edge_list and grating_list share: a list of square patches for a plane of side n as a tuple of parse(item),
    else ValueError. name = (article, noun) and square = (singular, plural) word the refusals, `holds` says what an item is. In this
    order: every item parses (TypeError or ValueError from parse: the whole list is refused); 1 .. most items; per item check(i, item)
    raises what is specific to the relation and returns the item's reach r, then the square centre +- r lies inside [0, n)^2; the
    squares are pairwise disjoint."""
    article, noun = name
    try:
        out = [parse(t) for t in items]
    except (TypeError, ValueError):
        raise ValueError("%s %s list holds %s, got %r" % (article, noun, holds, items))
    n = int(n)
    if not 1 <= len(out) <= most:
        raise ValueError("%s %s list holds 1 .. %d %ss, got %d" % (article, noun, most, noun, len(out)))
    squares = []
    for i, t in enumerate(out):
        x, y, r = t[0], t[1], check(i, t)
        if x - r < 0 or y - r < 0 or x + r >= n or y + r >= n:
            raise ValueError("%s %d: the %s (%d, %d) +- %d leaves the %d x %d plane" % (noun, i, square[0], x, y, r, n, n))
        squares.append((x, y, r))
    a = np.array(squares, dtype=np.int64)
    both = a[:, 2][:, None] + a[:, 2][None, :]
    meet = (np.abs(a[:, 0][:, None] - a[:, 0][None, :]) <= both) & (np.abs(a[:, 1][:, None] - a[:, 1][None, :]) <= both)
    np.fill_diagonal(meet, False)
    if meet.any():
        i, j = np.argwhere(meet)[0]
        raise ValueError("the %s of %ss %d and %d are not disjoint" % (square[1], noun, i, j))
    return tuple(out)


def detail_list(details, n, with_contrast=True):
    """The details (x, y, r, c) of a contrast-detail list for a plane of side n as harness.insert_details, harness.detail_statistics and
    the library take it, a tuple of tuples of ints, else ValueError: 1 .. DETAIL_MAX details of integers, 1 <= r <= DETAIL_MAX_RADIUS,
    1 <= |c| <= DETAIL_MAX_CONTRAST (with_contrast=False: c is not looked at, as the measurement does not), every box |px - x|,
    |py - y| <= 2r + 2 inside [0, n)^2 and the boxes pairwise disjoint."""
    def check(i, d):
        x, y, r, c = d
        if not 1 <= r <= DETAIL_MAX_RADIUS:
            raise ValueError("detail %d: radius %d is not in 1 .. %d" % (i, r, DETAIL_MAX_RADIUS))
        if with_contrast and not 1 <= abs(c) <= DETAIL_MAX_CONTRAST:
            raise ValueError("detail %d: contrast %d is not 1 <= |c| <= %d" % (i, c, DETAIL_MAX_CONTRAST))
        return 2 * r + 2
    return _patch_list(details, n, ("a", "detail"), "quadruples of integers (x, y, r, c)", DETAIL_MAX, lambda d: _ints(d, 4), check, ("box", "boxes"))


class Detail(C.Structure):
    """musica_detail: a disc of `radius` about the integer pixel centre (x, y), of `contrast` / 1024."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("radius", C.c_uint32), ("contrast", C.c_int32)]


DETAIL_ZONES = ("disc", "ring")   # index 0 and 1 of a musica_sim_detail_result's pairs
DETAIL_SUMS = ("n", "sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab")


class SimDetailResult(C.Structure):
    """musica_sim_detail_result: the exact sums of one detail's disc, ring and box."""
    _fields_ = [(k, C.c_uint64 * 2) for k in DETAIL_SUMS] + [("box_ssd", C.c_uint64), ("box_pixels", C.c_uint64)]

    def as_dict(self):
        d = {zone: {k: int(getattr(self, k)[i]) for k in DETAIL_SUMS} for i, zone in enumerate(DETAIL_ZONES)}
        d.update(box_ssd=int(self.box_ssd), box_pixels=int(self.box_pixels))
        return d


def edge_bins(h, p, q):
    """musica_edge_bins: the bins 2B + 1 of the edge-spread table of an edge of half-side h and slope p / q, B = ceil(4 (q + p) h / q);
    0 for an inadmissible triple (8 <= h <= EDGE_MAX_HALF, 1 <= p < q, 4 <= q <= EDGE_MAX_Q, gcd(p, q) = 1)."""
    h, p, q = int(h), int(p), int(q)
    if not (EDGE_MIN_HALF <= h <= EDGE_MAX_HALF and EDGE_MIN_Q <= q <= EDGE_MAX_Q and 1 <= p < q and math.gcd(p, q) == 1):
        return 0
    return 2 * (-((-4 * (q + p) * h) // q)) + 1


def edge_list(edges, n, with_contrast=True):
    """The edges (x, y, h, p, q, o, c) of a slanted-edge list for a plane of side n as harness.insert_edges, harness.edge_statistics and
    the library take it, a tuple of tuples of ints, else ValueError: 1 .. EDGE_MAX edges of integers, 8 <= h <= EDGE_MAX_HALF, a slope
    p / q with 1 <= p < q, 4 <= q <= EDGE_MAX_Q in lowest terms, an orientation o of 0 .. 3, 1 <= |c| <= EDGE_MAX_CONTRAST
    (with_contrast=False: c is not looked at, as the measurement does not), every plate |px - x|, |py - y| <= 2h inside [0, n)^2 and
    the plates pairwise disjoint."""
    def check(i, e):
        x, y, h, p, q, o, c = e
        if not EDGE_MIN_HALF <= h <= EDGE_MAX_HALF:
            raise ValueError("edge %d: half-side %d is not in %d .. %d" % (i, h, EDGE_MIN_HALF, EDGE_MAX_HALF))
        if not edge_bins(h, p, q):
            raise ValueError("edge %d: slope %d / %d is not 1 <= p < q, %d <= q <= %d in lowest terms" % (i, p, q, EDGE_MIN_Q, EDGE_MAX_Q))
        if not 0 <= o <= 3:
            raise ValueError("edge %d: orientation %d is not in 0 .. 3" % (i, o))
        if with_contrast and not 1 <= abs(c) <= EDGE_MAX_CONTRAST:
            raise ValueError("edge %d: contrast %d is not 1 <= |c| <= %d" % (i, c, EDGE_MAX_CONTRAST))
        return 2 * h
    return _patch_list(edges, n, ("an", "edge"), "septuples of integers (x, y, h, p, q, o, c)", EDGE_MAX, lambda e: _ints(e, 7), check, ("plate", "plates"))


class Edge(C.Structure):
    """musica_edge: a slanted edge of slope p / q and orientation o through the integer pixel centre (x, y), measured over
    |dx|, |dy| <= half and inserted over |dx|, |dy| <= 2 half with `contrast` / 1024."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("half", C.c_uint32), ("p", C.c_uint32), ("q", C.c_uint32), ("orientation", C.c_uint32),
                ("contrast", C.c_int32)]


EDGE_SUMS = ("n", "sum_a", "sum_b", "sum_aa")   # the four rows of an edge's table


class SimEdgeResult(C.Structure):
    """musica_sim_edge_result: the region's exact sum of squared differences and where the edge's table lies in `tables`."""
    _fields_ = [("roi_ssd", C.c_uint64), ("roi_pixels", C.c_uint64), ("table_offset", C.c_uint64), ("bins", C.c_uint64)]


def grating_admissible(half, ux, uy, period):
    """Whether (half, ux, uy, T) is a grating's geometry: GRATING_MIN_HALF <= half <= GRATING_MAX_HALF, |ux|, |uy| <= GRATING_MAX_U, not
    both 0, gcd(|ux|, |uy|) = 1, 2 <= T <= GRATING_MAX_PERIOD, T <= half, 2 |ux| <= T and 2 |uy| <= T."""
    return (GRATING_MIN_HALF <= half <= GRATING_MAX_HALF and abs(ux) <= GRATING_MAX_U and abs(uy) <= GRATING_MAX_U and math.gcd(abs(ux), abs(uy)) == 1 and
            2 <= period <= min(GRATING_MAX_PERIOD, half) and 2 * abs(ux) <= period and 2 * abs(uy) <= period)


def grating_list(gratings, n, with_wave=True):
    """The gratings (x, y, h, ux, uy, T, wave) of a grating list for a plane of side n as harness.insert_gratings,
    harness.grating_statistics and the library take it, a tuple of tuples of ints whose last element is the wave as a tuple of T ints,
    else ValueError: 1 .. GRATING_MAX gratings of integers, 8 <= h <= GRATING_MAX_HALF, a wave vector (ux, uy) with |ux|, |uy| <=
    GRATING_MAX_U, not both 0 and coprime, a period 2 <= T <= min(GRATING_MAX_PERIOD, h) with 2 |ux| <= T and 2 |uy| <= T, a wave of
    exactly T integers |w| <= GRATING_MAX_CONTRAST (with_wave=False: the wave is not looked at, as the measurement does not, and comes
    back as it was given), every plate |px - x|, |py - y| <= 2h inside [0, n)^2 and the plates pairwise disjoint."""
    def parse(g):
        g = tuple(g)
        if len(g) != 7:
            raise TypeError
        return _ints(g[:6], 6) + (_ints(g[6], len(g[6])) if with_wave else g[6],)

    def check(i, g):
        x, y, h, ux, uy, t, wave = g
        if not GRATING_MIN_HALF <= h <= GRATING_MAX_HALF:
            raise ValueError("grating %d: half-side %d is not in %d .. %d" % (i, h, GRATING_MIN_HALF, GRATING_MAX_HALF))
        if not (abs(ux) <= GRATING_MAX_U and abs(uy) <= GRATING_MAX_U and math.gcd(abs(ux), abs(uy)) == 1):
            raise ValueError("grating %d: wave vector (%d, %d) is not coprime with |ux|, |uy| <= %d" % (i, ux, uy, GRATING_MAX_U))
        if not grating_admissible(h, ux, uy, t):
            raise ValueError("grating %d: period %d is not 2 <= T <= min(%d, half) with 2 |ux|, 2 |uy| <= T" % (i, t, GRATING_MAX_PERIOD))
        if with_wave and (len(wave) != t or any(abs(w) > GRATING_MAX_CONTRAST for w in wave)):
            raise ValueError("grating %d: the wave is not %d integers |w| <= %d" % (i, t, GRATING_MAX_CONTRAST))
        return 2 * h
    return _patch_list(gratings, n, ("a", "grating"), "septuples (x, y, h, ux, uy, T, wave) of six integers and a sequence of integers", GRATING_MAX,
                       parse, check, ("plate", "plates"))


class Grating(C.Structure):
    """musica_grating: a grating of wave vector (ux, uy) and period T about the integer pixel centre (x, y), measured over
    |dx|, |dy| <= half and inserted over |dx|, |dy| <= 2 half."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("half", C.c_uint32), ("ux", C.c_int32), ("uy", C.c_int32), ("period", C.c_uint32)]


GRATING_SUMS = ("n", "sum_a", "sum_b", "sum_aa")   # the four rows of a grating's table


class SimGratingResult(C.Structure):
    """musica_sim_grating_result: the region's exact sum of squared differences and where the grating's table lies in `tables`."""
    _fields_ = [("roi_ssd", C.c_uint64), ("roi_pixels", C.c_uint64), ("table_offset", C.c_uint64), ("bins", C.c_uint64)]


def point_list(points, n, with_contrast=True):
    """The points (x, y, R, s, c, group) of a point-response list for a plane of side n as harness.insert_points,
    harness.point_statistics and the library take it, a tuple of tuples of ints, else ValueError: 1 .. POINT_MAX points of integers,
    POINT_MIN_RADIUS <= R <= POINT_MAX_RADIUS and the same R for every point, a cluster size 1 <= s <= POINT_MAX_SIZE,
    POINT_MIN_CONTRAST <= c <= POINT_MAX_CONTRAST and c != 0 (with_contrast=False: c is not looked at, as the measurement does not), a
    group in 0 .. POINT_MAX_GROUPS - 1, every window |px - x|, |py - y| <= R inside [0, n)^2 and the windows pairwise disjoint."""
    first = []

    def check(i, p):
        x, y, r, s, c, g = p
        if not POINT_MIN_RADIUS <= r <= POINT_MAX_RADIUS:
            raise ValueError("point %d: radius %d is not in %d .. %d" % (i, r, POINT_MIN_RADIUS, POINT_MAX_RADIUS))
        first.append(r)
        if r != first[0]:
            raise ValueError("point %d: radius %d differs from the list's radius %d" % (i, r, first[0]))
        if not 1 <= s <= POINT_MAX_SIZE:
            raise ValueError("point %d: size %d is not in 1 .. %d" % (i, s, POINT_MAX_SIZE))
        if with_contrast and (c == 0 or not POINT_MIN_CONTRAST <= c <= POINT_MAX_CONTRAST):
            raise ValueError("point %d: contrast %d is not in %d .. %d without 0" % (i, c, POINT_MIN_CONTRAST, POINT_MAX_CONTRAST))
        if not 0 <= g < POINT_MAX_GROUPS:
            raise ValueError("point %d: group %d is not in 0 .. %d" % (i, g, POINT_MAX_GROUPS - 1))
        return r
    return _patch_list(points, n, ("a", "point"), "sextuples of integers (x, y, R, s, c, group)", POINT_MAX, lambda p: _ints(p, 6), check, ("window", "windows"))


def point_groups(points, groups=None):
    """How many stacks the measurement of a checked point list keeps: `groups`, by default 1 + the largest group of the list; an integer
    in 1 .. POINT_MAX_GROUPS above every point's group, else ValueError."""
    most = max(p[5] for p in points)
    if groups is None:
        return most + 1
    if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or not 1 <= groups <= POINT_MAX_GROUPS:
        raise ValueError("groups %r is not an integer in 1 .. %d" % (groups, POINT_MAX_GROUPS))
    if most >= groups:
        raise ValueError("a point's group %d is not below groups %d" % (most, groups))
    return int(groups)


class Defect(C.Structure):
    """musica_defect: a cluster of `size` x `size` pixels at the integer pixel centre (x, y) altered by `contrast` / 1024, measured over
    the window |dx|, |dy| <= `radius` and stacked with the other points of its `group`. (Point is the curves' (x, y).)"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("radius", C.c_uint32), ("size", C.c_uint32), ("contrast", C.c_int32), ("group", C.c_uint32)]


POINT_SUMS = ("core_sum_a", "core_sum_b", "win_sum_a", "win_sum_b", "win_ssd", "win_pixels")   # a musica_sim_point_result's words
POINT_STACKS = ("sum_a", "sum_b", "ssd")                                                       # the three planes of a group's stack


class SimPointResult(C.Structure):
    """musica_sim_point_result: the exact sums of one point's core and window."""
    _fields_ = [(k, C.c_uint64) for k in POINT_SUMS]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in POINT_SUMS}


def view_list(views, banks, n):
    """The views (x, y, bank) and the template banks of a model-observer call for a plane of side n as metrics.channel_responses and the
    library take them: (a tuple of tuples of ints, a tuple of contiguous int8 arrays (C, S, S)), else ValueError, checked as the C side
    checks: 1 .. OBSERVER_MAX_BANKS banks, each an array of integers within int8 of shape (C, S, S) with 1 <= C <= OBSERVER_MAX_CHANNELS
    and S = 2 half + 1, 1 <= half <= OBSERVER_MAX_HALF; 1 .. OBSERVER_MAX_VIEWS views of integers, each naming a bank of the call and
    with its window |px - x|, |py - y| <= half inside [0, n)^2. The windows may overlap and views may repeat."""
    try:
        arrays = [np.asarray(b) for b in banks]
    except (TypeError, ValueError):
        raise ValueError("the banks are a sequence of integer arrays (C, S, S), got %r" % (banks,))
    if not 1 <= len(arrays) <= OBSERVER_MAX_BANKS:
        raise ValueError("an observer call holds 1 .. %d banks, got %d" % (OBSERVER_MAX_BANKS, len(arrays)))
    out_banks = []
    for k, a in enumerate(arrays):
        if a.ndim != 3 or a.shape[1] != a.shape[2] or a.dtype.kind not in "iu" or not a.size:
            raise ValueError("bank %d: not a (C, S, S) array of integers, got %r %s" % (k, a.shape, a.dtype))
        if a.shape[1] % 2 != 1 or not 1 <= a.shape[1] // 2 <= OBSERVER_MAX_HALF:
            raise ValueError("bank %d: side %d is not 2 half + 1 with half in 1 .. %d" % (k, a.shape[1], OBSERVER_MAX_HALF))
        if not 1 <= a.shape[0] <= OBSERVER_MAX_CHANNELS:
            raise ValueError("bank %d: %d channels are not in 1 .. %d" % (k, a.shape[0], OBSERVER_MAX_CHANNELS))
        if int(a.min()) < -128 or int(a.max()) > 127:
            raise ValueError("bank %d: a weight is beyond int8" % k)
        out_banks.append(np.ascontiguousarray(a, dtype=np.int8))
    try:
        out = [_ints(v, 3) for v in views]
    except (TypeError, ValueError):
        raise ValueError("a view list holds triples of integers (x, y, bank), got %r" % (views,))
    n = int(n)
    if not 1 <= len(out) <= OBSERVER_MAX_VIEWS:
        raise ValueError("a view list holds 1 .. %d views, got %d" % (OBSERVER_MAX_VIEWS, len(out)))
    for i, (x, y, k) in enumerate(out):
        if not 0 <= k < len(out_banks):
            raise ValueError("view %d: bank %d is not in 0 .. %d" % (i, k, len(out_banks) - 1))
        r = out_banks[k].shape[1] // 2
        if x - r < 0 or y - r < 0 or x + r >= n or y + r >= n:
            raise ValueError("view %d: the window (%d, %d) +- %d leaves the %d x %d plane" % (i, x, y, r, n, n))
    return tuple(out), tuple(out_banks)


class ChannelBank(C.Structure):
    """musica_channel_bank: `channels` int8 templates over the window |dx|, |dy| <= half, weights[channels][S][S]."""
    _fields_ = [("half", C.c_uint32), ("channels", C.c_uint32), ("weights", C.POINTER(C.c_int8))]


class View(C.Structure):
    """musica_view: a window of bank `bank` about the integer pixel centre (x, y)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("bank", C.c_uint32)]


class SimObserverResult(C.Structure):
    """musica_sim_observer_result: where a view's responses lie in `tables`, its window's pixel count and plain sums."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint32), ("sum_a", C.c_uint32), ("sum_b", C.c_uint32)]


def _unpack_tables(results, tables, sums):
    """Per musica_sim_edge_result / musica_sim_grating_result: (its bins, {roi_ssd, roi_pixels and the uint32 arrays `sums`, the rows
    of its [len(sums)][bins] table in the flat `tables`})."""
    out = []
    for r in results:
        at, bins = int(r.table_offset), int(r.bins)
        t = tables[at:at + len(sums) * bins].reshape(len(sums), bins)
        d = {"roi_ssd": int(r.roi_ssd), "roi_pixels": int(r.roi_pixels)}
        d.update((k, t[i].copy()) for i, k in enumerate(sums))
        out.append((bins, d))
    return out


def gain_tables(gx, gy, n):
    """The two tables of a gain map for a plane of side n as harness.apply_gain and the library take them: (gx, gy), uint16 arrays of n
    entries (columns, rows) in units of 1 / GAIN_ONE, else ValueError: each a sequence of n integers in 0 .. 65535."""
    out = []
    for name, g in (("gx", gx), ("gy", gy)):
        a = np.asarray(g)
        if a.ndim != 1 or a.shape[0] != int(n) or a.dtype.kind not in "iu" or (a.size and (int(a.min()) < 0 or int(a.max()) > 65535)):
            raise ValueError("%s is not %d integers in 0 .. 65535, got %r %s" % (name, int(n), a.shape, a.dtype))
        out.append(np.ascontiguousarray(a, dtype=np.uint16))
    return tuple(out)


PROFILE_SUMS = ("sum_a", "sum_b", "sum_dd", "sum_aa")   # the four words of a line of a profile table


class SimProfileResult(C.Structure):
    """musica_sim_profile_result: where a query's column and row tables lie in `tables`, and the region's exact sum of squared differences."""
    _fields_ = [("table_offset", C.c_uint64), ("cols", C.c_uint64), ("rows", C.c_uint64), ("ssd", C.c_uint64), ("pixels", C.c_uint64)]


def lut_table(lut):
    """A tone table as harness.apply_lut and the library take it: a uint16 array of LUT_ENTRIES entries, else ValueError: a sequence of
    LUT_ENTRIES integers in 0 .. 65535."""
    a = np.asarray(lut)
    if a.ndim != 1 or a.shape[0] != LUT_ENTRIES or a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 65535:
        raise ValueError("lut is not %d integers in 0 .. 65535, got %r %s" % (LUT_ENTRIES, a.shape, a.dtype))
    return np.ascontiguousarray(a, dtype=np.uint16)


def level_count(shift):
    """How many classes source >> shift has, (65535 >> shift) + 1 <= 4096, for an integer shift in LEVEL_MIN_SHIFT .. LEVEL_MAX_SHIFT,
    else ValueError."""
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not LEVEL_MIN_SHIFT <= shift <= LEVEL_MAX_SHIFT:
        raise ValueError("shift %r is not an integer in %d .. %d" % (shift, LEVEL_MIN_SHIFT, LEVEL_MAX_SHIFT))
    return (65535 >> int(shift)) + 1


LEVEL_SUMS = ("n", "sum_a", "sum_b", "sum_dd", "sum_aa", "sum_bb")   # the six words of a class of a level table


class SimLevelResult(C.Structure):
    """musica_sim_level_result: where a query's table lies in `tables`, and the region's exact sum of squared differences."""
    _fields_ = [("table_offset", C.c_uint64), ("classes", C.c_uint64), ("ssd", C.c_uint64), ("pixels", C.c_uint64)]


GRADIENT_FIELDS = ("n", "sum_A", "sum_B", "sum_dot", "sum_cross", "neg")   # the six words of a class of a gradient table


class SimGradientResult(C.Structure):
    """musica_sim_gradient_result: where a query's table lies in `tables`, the interior's pixel count and the mean of q."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint64), ("gsim", C.c_double)]


REACH_FIELDS = ("n", "changed", "sum_a", "sum_b", "sum_dd", "max_d")   # the six words of a class of a reach table


class SimReachResult(C.Structure):
    """musica_sim_reach_result: where a query's table lies in `tables`, the region's exact sum of squared differences and the number
    of changed pixels of the whole input plane."""
    _fields_ = [("table_offset", C.c_uint64), ("classes", C.c_uint64), ("ssd", C.c_uint64), ("pixels", C.c_uint64), ("seeds", C.c_uint64)]


def reach_radii(radii):
    """A list of reach radii as metrics.reach_classes and the library take it: a uint32 array of 1 .. REACH_MAX_RADII integers, the first
    0, strictly ascending, each at most REACH_MAX_RADIUS, else ValueError."""
    r = [v for v in radii]
    if not 1 <= len(r) <= REACH_MAX_RADII or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in r):
        raise ValueError("radii are not 1 .. %d integers, got %r" % (REACH_MAX_RADII, r))
    r = [int(v) for v in r]
    if r[0] != 0 or any(b <= a for a, b in zip(r, r[1:])) or r[-1] > REACH_MAX_RADIUS:
        raise ValueError("radii do not ascend strictly from 0 to at most %d: %r" % (REACH_MAX_RADIUS, r))
    return np.array(r, dtype=np.uint32)


ORDER_FIELDS = ("pairs", "same", "reversed", "flattened", "split")   # the five words of a ring of an order table (MUSICA_ORDER_WORDS)
ORDER_TABLE_WORDS = ORDER_RINGS * len(ORDER_FIELDS) + ORDER_BINS      # MUSICA_ORDER_TABLE_WORDS = 112


class SimOrderResult(C.Structure):
    """musica_sim_order_result: where a query's table lies in `tables` and the interior's pixel count."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint64)]


LATTICE_FIELDS = ("n", "sum_a", "sum_b", "sum_dd", "step_x_a", "step_x_b", "step_y_a", "step_y_b")   # the eight words of a class of a lattice table (MUSICA_LATTICE_WORDS)


class SimLatticeResult(C.Structure):
    """musica_sim_lattice_result: where a query's table lies in `tables` and the number of counted pixels."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint64)]


BLOB_FIELDS = ("components", "pixels", "sum_d", "sum_dd", "box_area", "border")   # the six words of a class of a blob table (MUSICA_BLOB_WORDS)


SPECTRUM_FIELDS = ("sum_aa", "sum_bb", "sum_ab")   # the three words of a coefficient of a spectrum table (MUSICA_SPECTRUM_WORDS)


class SimSpectrumResult(C.Structure):
    """musica_sim_spectrum_result: where a query's table lies in `tables` and the number of whole tiles."""
    _fields_ = [("table_offset", C.c_uint64), ("tiles", C.c_uint64)]


class SimCooccurrenceResult(C.Structure):
    """musica_sim_cooccurrence_result: where a query's tables lie in `tables` and the pairs of every [distance][direction]."""
    _fields_ = [("table_offset", C.c_uint64), ("pairs", (C.c_uint64 * 4) * COOCCURRENCE_MAX_DISTANCES)]


class SimGranulometryResult(C.Structure):
    """musica_sim_granulometry_result: where a query's table lies in `tables` and the pixels of its region."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint64)]


class SimContoursResult(C.Structure):
    """musica_sim_contours_result: where a query's table and byte plane lie, the sizes of its two contour sets and its pixels."""
    _fields_ = [("table_offset", C.c_uint64), ("contour_a", C.c_uint64), ("contour_b", C.c_uint64), ("pixels", C.c_uint64), ("plane_offset", C.c_uint64)]


class SimMinkowskiResult(C.Structure):
    """musica_sim_minkowski_result: where a query's table lies and its pixels."""
    _fields_ = [("table_offset", C.c_uint64), ("pixels", C.c_uint64)]


class SimBlobsResult(C.Structure):
    """musica_sim_blobs_result: where a query's table and label plane lie, its counts and its largest component."""
    _fields_ = [("table_offset", C.c_uint64), ("label_offset", C.c_uint64), ("pixels", C.c_uint64), ("changed", C.c_uint64), ("components", C.c_uint64),
                ("largest_sum_dd", C.c_uint64), ("largest_n", C.c_uint32), ("largest_first", C.c_uint32), ("largest_x0", C.c_uint32), ("largest_y0", C.c_uint32),
                ("largest_x1", C.c_uint32), ("largest_y1", C.c_uint32)]


class SimDisplaceResult(C.Structure):
    """musica_sim_displace_result: where one comparison's exact block matching puts the output."""
    _fields_ = [("pixels", C.c_uint64), ("ssd_zero", C.c_uint64), ("ssd_min", C.c_uint64), ("dx", C.c_int32), ("dy", C.c_int32),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("tiles_off", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


SIM_MAX_SCALES = 5          # MUSICA_SIM_MAX_SCALES
SCALE_METRICS = ("ssim", "cs", "lum", "mse")   # the per-scale lists of harness.multiscale_similarities (beside ms_ssim and scales)


class SimScalesResult(C.Structure):
    """musica_sim_scales_result: the scale-resolved SSIM of one comparison."""
    _fields_ = [("scales", C.c_uint32), ("pixels", C.c_uint64), ("ms_ssim", C.c_double)] + \
               [(n, C.c_double * SIM_MAX_SCALES) for n in SCALE_METRICS] + \
               [("ssd", C.c_uint64 * SIM_MAX_SCALES), ("plane_w", C.c_uint32 * SIM_MAX_SCALES), ("plane_h", C.c_uint32 * SIM_MAX_SCALES)]

    def as_dict(self):
        """The entries of the scales asked for; "raw": every array at its full length (zero beyond them)."""
        n = int(self.scales)
        d = {"scales": n, "pixels": int(self.pixels), "ms_ssim": float(self.ms_ssim)}
        for k in SCALE_METRICS:
            d[k] = [float(v) for v in getattr(self, k)[:n]]
        for k in ("ssd", "plane_w", "plane_h"):
            d[k] = [int(v) for v in getattr(self, k)[:n]]
        d["raw"] = {k: list(getattr(self, k)) for k in SCALE_METRICS + ("ssd", "plane_w", "plane_h")}
        return d


SIM_ENSEMBLE_MAX = 1024     # MUSICA_SIM_ENSEMBLE_MAX
ENSEMBLE_METRICS = ("mean_shift", "bias_rms", "noise_rms", "mse", "bias_fraction")                      # the doubles of an ensemble result
ENSEMBLE_INTEGERS = ("sq_bias_sum", "var_sum", "sq_err_sum", "bias_sum", "abs_bias_max", "var_max",      # its exact integers
                     "pixels", "realisations", "tiles_x", "tiles_y")


class SimEnsembleResult(C.Structure):
    """musica_sim_ensemble_stats: the ensemble statistics of one query (harness.ensemble_statistics' keys)."""
    _fields_ = [(n, C.c_double) for n in ENSEMBLE_METRICS] + \
               [("sq_bias_sum", C.c_uint64), ("var_sum", C.c_uint64), ("sq_err_sum", C.c_uint64), ("bias_sum", C.c_int64),
                ("abs_bias_max", C.c_uint64), ("var_max", C.c_uint64), ("pixels", C.c_uint64),
                ("realisations", C.c_uint32), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32)]

    def as_dict(self):
        d = {n: float(getattr(self, n)) for n in ENSEMBLE_METRICS}
        d.update({n: int(getattr(self, n)) for n in ENSEMBLE_INTEGERS})
        return d


SIM_COV_MAX_REGIONS = 4     # MUSICA_SIM_COV_MAX_REGIONS
COV_METRICS = ("noise_var", "rho_x", "rho_y", "corr_area")                                  # the doubles of a covariance result
COV_INTEGERS = ("c00", "pixels", "realisations", "radius", "tiles_x", "tiles_y")            # its exact integers


class SimCovResult(C.Structure):
    """musica_sim_cov_result: the noise covariance summary of one tracked region (harness.ensemble_covariance's keys)."""
    _fields_ = [(n, C.c_double) for n in COV_METRICS] + \
               [("c00", C.c_int64), ("pixels", C.c_uint64), ("realisations", C.c_uint32), ("radius", C.c_uint32),
                ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32)]

    def as_dict(self):
        d = {n: float(getattr(self, n)) for n in COV_METRICS}
        d.update({n: int(getattr(self, n)) for n in COV_INTEGERS})
        return d


# musica_out_format: what export_out writes per image
OUT_U8, OUT_GRADED_F32 = 0, 1
OUT_FORMAT_COUNT = 2


def out_geometry(image_size, fmt):
    """(rows, bytes per row) of one image of export_out: (N - 20, N - 20) for OUT_U8, (N, 4 N) for OUT_GRADED_F32."""
    if fmt == OUT_U8:
        side = max(image_size - 2 * OUT_MARGIN, 0)
        return side, side
    return image_size, 4 * image_size


# musica_alteration_kind
ALTER_NONE, ALTER_TRANSLATE, ALTER_ROTATE, ALTER_COLLIMATOR, ALTER_GAUSSIAN, ALTER_POISSON, ALTER_SYMMETRY = range(7)
ALTER_KIND_COUNT = 7


class Alteration(C.Structure):
    """musica_alteration: one of the study's alterations (include/musica.h)."""
    _fields_ = [("kind", C.c_uint32), ("dx", C.c_int32), ("dy", C.c_int32), ("margin", C.c_int32), ("shutter_h", C.c_int32),
                ("shutter_v", C.c_int32), ("mean", C.c_double), ("sigma", C.c_double), ("factor", C.c_double), ("seed", C.c_uint64),
                ("stream", C.c_uint32), ("matrix", C.c_double * 4), ("offset", C.c_double * 2)]


def rotation_params(side, degree):
    """(matrix, offset) of ndimage.rotate(reshape=False) for a side x side plane, computed the way scipy computes them (special.cosdg /
    sindg, offset = in_center - rot_matrix @ out_center, in numpy), so the device mapping sees the same doubles."""
    from scipy import special
    c, s = special.cosdg(degree), special.sindg(degree)
    rot_matrix = np.array([[c, s], [-s, c]])
    shape = np.asarray((side, side))
    out_center = rot_matrix @ ((shape - 1) / 2)
    in_center = (shape - 1) / 2
    return rot_matrix, in_center - out_center


# Every symbol include/musica.h declares: (restype, argtypes). tests/test_abi.py checks the
# shared object exports exactly these.
_VP = C.c_void_p
_U8P, _U16P, _U32P, _F32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
ABI = {
    "musica_create": (_VP, [C.POINTER(Params)]),
    "musica_destroy": (None, [_VP]),
    "musica_get_image_size": (C.c_uint32, [_VP]),
    "musica_get_levels": (C.c_uint32, [_VP]),
    "musica_get_batch": (C.c_uint32, [_VP]),
    "musica_get_level_size": (C.c_uint32, [_VP, C.c_uint32]),
    "musica_fuses_gradation_histogram": (C.c_int, [_VP]),
    "musica_fuses_reduce_band": (C.c_int, [_VP]),
    "musica_fuses_sdev": (C.c_int, [_VP]),
    "musica_get_paired_levels": (C.c_int, [_VP]),
    "musica_fuses_noise_hist": (C.c_int, [_VP]),
    "musica_get_dispatch": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "musica_execute": (C.c_int, [_VP, _U16P]),
    "musica_execute_device": (C.c_int, [_VP, _VP]),
    "musica_execute_stream": (C.c_int, [_VP, C.POINTER(_VP), C.c_uint32, C.POINTER(Stats)]),
    "musica_host_alloc": (_VP, [_VP, C.c_size_t]),
    "musica_host_free": (None, [_VP, _VP]),
    "musica_upload": (C.c_int, [_VP, _U16P]),
    "musica_input_device_ptr": (_VP, [_VP]),
    "musica_sync": (C.c_int, [_VP]),
    "musica_get_graded": (C.c_int, [_VP, _F32P]),
    "musica_save_out_image": (C.c_int, [_VP, C.c_uint32, C.c_char_p]),
    "musica_get_out_pixels": (C.c_int, [_VP, C.c_uint32, _U8P]),
    "musica_get_image": (C.c_int, [_VP, C.c_uint32, C.c_int, C.c_uint32, _F32P]),
    "musica_image_side": (C.c_uint32, [_VP, C.c_int, C.c_uint32]),
    "musica_get_noise_hist": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _U32P]),
    "musica_get_grad_hist": (C.c_int, [_VP, C.c_uint32, _U32P]),
    "musica_get_noise_hist_max": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(HistMaxPoint)]),
    "musica_get_grad_hist_max": (C.c_int, [_VP, C.c_uint32, C.POINTER(HistMaxPoint)]),
    "musica_get_contrast_curve": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(ContrastCurve)]),
    "musica_get_grad_curve": (C.c_int, [_VP, C.c_uint32, C.POINTER(GradCurve)]),
    "musica_get_contrast_params": (C.c_int, [_VP, C.c_uint32, C.POINTER(ContrastParams)]),
    "musica_get_nr_params": (C.c_int, [_VP, C.c_uint32, C.POINTER(NrParams)]),
    "musica_get_minmax": (C.c_int, [_VP, C.c_uint32, _F32P, _F32P]),
    "musica_get_stats": (C.c_int, [_VP, C.c_uint32, C.POINTER(Stats)]),
    "musica_stats_device": (C.c_int, [_VP, _VP, C.c_uint32]),
    "musica_stats_device_strided": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32]),
    "musica_get_clahe_hist": (C.c_int, [_VP, C.c_uint32, _U32P]),
    "musica_get_clahe_curves": (C.c_int, [_VP, C.c_uint32, C.POINTER(Point)]),
    "musica_debug_process": (C.c_int, [_VP, C.c_uint32, C.c_char_p]),
    "musica_render_noise_hist": (C.c_int, [_VP, C.c_uint32, _U8P]),
    "musica_render_grad_hist": (C.c_int, [_VP, C.c_uint32, _U8P]),
    "musica_debug_set_image": (C.c_int, [_VP, C.c_uint32, C.c_int, C.c_uint32, _F32P]),
    "musica_debug_run_stage": (C.c_int, [_VP, C.c_int]),
    "musica_profile_enable": (C.c_int, [_VP, C.c_int]),
    "musica_profile_reset": (C.c_int, [_VP]),
    "musica_profile_get": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "musica_k_reduce": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, _VP, C.c_uint32, C.c_uint32]),
    "musica_selftest_exact_math": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "musica_k_reduce_timed": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "musica_k_reduce_timed_rot": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "musica_k_copy41_timed_rot": (C.c_int, [_VP, _VP, C.c_uint32, _VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "musica_device_alloc": (_VP, [_VP, C.c_size_t]),
    "musica_device_free": (None, [_VP, _VP]),
    "musica_memcpy_h2d": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "musica_memcpy_d2h": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "musica_read_raw": (C.c_int, [C.c_char_p, C.c_uint32, _U16P]),
    "musica_write_bmp_gray": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _U8P]),
    "musica_write_bmp_rgba": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _U8P]),
    "musica_pipeline_create": (_VP, [C.POINTER(Params), C.c_uint32]),
    "musica_pipeline_destroy": (None, [_VP]),
    "musica_pipeline_depth": (C.c_uint32, [_VP]),
    "musica_pipeline_context": (_VP, [_VP, C.c_uint32]),
    "musica_pipeline_upload": (C.c_int, [_VP, _U16P]),
    "musica_pipeline_prime": (C.c_int, [_VP, C.c_uint32]),
    "musica_pipeline_calibration": (C.c_uint32, [_VP, _F32P]),
    "musica_pipeline_step": (C.c_int, [_VP, _VP]),
    "musica_pipeline_last": (_VP, [_VP]),
    "musica_pipeline_sync": (C.c_int, [_VP]),
    "musica_last_error": (C.c_char_p, []),
    "musica_abi_version": (C.c_uint32, []),
    "musica_create_ex": (_VP, [C.POINTER(Params), C.POINTER(Tunables)]),
    "musica_tunables_default": (None, [C.POINTER(Tunables)]),
    "musica_get_tunables": (C.c_int, [_VP, C.POINTER(Tunables)]),
    "musica_pipeline_create_ex": (_VP, [C.POINTER(Params), C.c_uint32, C.POINTER(Tunables)]),
    "musica_device_count": (C.c_int, []),
    "musica_sim_capture": (C.c_int, [_VP, C.c_uint32, C.c_uint32]),
    "musica_sim_set_reference": (C.c_int, [_VP, C.c_uint32, _U8P]),
    "musica_sim_set_vendor_reference": (C.c_int, [_VP, C.c_uint32, _VP, C.c_uint32]),
    "musica_sim_compare": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimResult)]),
    "musica_sim_rotate_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "musica_sim_get_reference": (C.c_int, [_VP, C.c_uint32, _U8P]),
    "musica_sim_transform_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_sim_blur_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_alter_blur": (C.c_int, [_VP, C.c_uint32, C.c_uint32]),
    "musica_sim_codec_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16), C.c_uint32]),
    "musica_alter_codec": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_uint16)]),
    "musica_sim_zoom_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_alter_zoom": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_sim_scatter_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_alter_scatter": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_sim_warp_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(C.c_int16), C.c_uint32, C.c_uint32]),
    "musica_alter_warp": (C.c_int, [_VP, C.c_uint32, C.POINTER(C.c_int16), C.c_uint32]),
    "musica_alter_details": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(Detail)]),
    "musica_sim_details": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Detail), C.POINTER(SimDetailResult)]),
    "musica_alter_edges": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(Edge)]),
    "musica_sim_edges": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Edge), C.POINTER(SimEdgeResult), _U32P, C.c_uint64]),
    "musica_edge_bins": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "musica_alter_gratings": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(Grating), C.POINTER(C.c_int16), C.c_uint64]),
    "musica_sim_gratings": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Grating), C.POINTER(SimGratingResult), _U32P, C.c_uint64]),
    "musica_alter_points": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(Defect)]),
    "musica_sim_points": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Defect), C.c_uint32, C.POINTER(SimPointResult), _U32P, C.c_uint64]),
    "musica_sim_observer": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ChannelBank), C.c_uint32, C.POINTER(View), C.POINTER(SimObserverResult),
                                      C.POINTER(C.c_int32), C.c_uint64]),
    "musica_alter_gain": (C.c_int, [_VP, C.c_uint32, _U16P, _U16P]),
    "musica_sim_profiles": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimProfileResult), _U32P, C.c_uint64]),
    "musica_alter_lut": (C.c_int, [_VP, C.c_uint32, _U16P]),
    "musica_sim_levels": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimLevelResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_gradients": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimGradientResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_reach": (C.c_int, [_VP, C.c_uint32, _U32P, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimReachResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_reach_classes": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _U32P, _U8P]),
    "musica_sim_order": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimOrderResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_lattice": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimLatticeResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_spectrum": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimSpectrumResult), C.POINTER(C.c_int64), C.c_uint64]),
    "musica_sim_cooccurrence": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _U32P, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimCooccurrenceResult), _U32P, C.c_uint64]),
    "musica_sim_granulometry": (C.c_int, [_VP, C.c_uint32, _U32P, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimGranulometryResult), C.POINTER(C.c_uint64), C.c_uint64]),
    "musica_sim_contours": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimContoursResult), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64]),
    "musica_sim_minkowski": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimMinkowskiResult), _U32P, C.c_uint64]),
    "musica_sim_blobs": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimBlobsResult), C.POINTER(C.c_uint64), C.c_uint64, _U32P, C.c_uint64]),
    "musica_sim_joint": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimJointResult), _U32P]),
    "musica_sim_displace": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.c_uint32, C.POINTER(SimDisplaceResult), C.POINTER(C.c_uint64), _U32P]),
    "musica_sim_remap_reference": (C.c_int, [_VP, C.c_uint32, C.c_uint32, _U8P]),
    "musica_sim_multiscale": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.c_uint32, C.POINTER(SimScalesResult)]),
    "musica_sim_ensemble_reset": (C.c_int, [_VP]),
    "musica_sim_ensemble_add": (C.c_int, [_VP, C.c_uint32, C.c_uint32]),
    "musica_sim_ensemble_result": (C.c_int, [_VP, C.c_uint32, C.POINTER(SimQuery), C.POINTER(SimEnsembleResult), C.POINTER(C.c_uint64)]),
    "musica_sim_ensemble_get": (C.c_int, [_VP, _U32P, _U32P, _U32P]),
    "musica_sim_ensemble_track": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.POINTER(SimQuery)]),
    "musica_sim_ensemble_covariance": (C.c_int, [_VP, C.POINTER(SimCovResult), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "musica_alter_set_source": (C.c_int, [_VP, _U16P]),
    "musica_alter": (C.c_int, [_VP, C.c_uint32, C.POINTER(Alteration)]),
    "musica_alter_draws": (C.c_int, [_VP, C.POINTER(Alteration), C.POINTER(C.c_int32)]),
    "musica_alter_percentile": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_double)]),
    "musica_export_out": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32, _VP, C.c_size_t, C.c_size_t]),
    "musica_stream_wait": (C.c_int, [_VP, _VP]),
    "musica_stream_signal": (C.c_int, [_VP, _VP]),
}

_lib = None


def load_library():
    """Load libmusica_hip.so (built in-tree by build.py). Raises if it is missing: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libmusica_hip.so is not built: run `python -m %s.build` (hipcc, gfx950)" % __package__)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return (load_library().musica_last_error() or b"").decode("utf-8", "replace")


def device_count():
    return load_library().musica_device_count()


def _f32p(a):
    return a.ctypes.data_as(_F32P)


def _queries(queries):
    """The queries of a call as SimQuery: one passes through, any other sequence of its eight fields goes through int() field by field."""
    return [q if isinstance(q, SimQuery) else SimQuery(*[int(v) for v in q]) for q in queries]


class MusicaProcessing:
    """Drop-in for the reference's VulkanProcessing (one HIP stream on one device per object)."""

    def __init__(self, device=0):
        # reference: VulkanProcessing(VulkanState*) — the state object selected the physical device
        self._lib = load_library()
        self._device = int(device)
        self._h = None
        self._owned = True
        self.imageSize = 0
        self.pyramidLevels = 0
        self.batch = 1

    @classmethod
    def _borrow(cls, handle, device=0):
        """A view of a context something else owns (a MusicaPipeline): every getter works, cleanup() leaves it alone."""
        self = cls(device)
        self._h = handle
        self._owned = False
        self.imageSize = self._lib.musica_get_image_size(handle)
        self.pyramidLevels = self._lib.musica_get_levels(handle)
        self.batch = self._lib.musica_get_batch(handle)
        return self

    # ---- the reference's interface -------------------------------------------------
    def init(self, imageSize, outImageViews=None, levels=0, batch=1, flags=0, tunables=None):
        """bool init(uint32_t imageSize, std::vector<VkImageView>*) — src/vk_processing.cpp:1984-2020.
        tunables: a Tunables (default_tunables(...)) — the reference's compile-time constants as runtime values; None = the reference's."""
        if self._h:
            self.cleanup()
        p = Params(int(imageSize), int(levels), int(batch), self._device, int(flags))
        h = self._lib.musica_create_ex(C.byref(p), C.byref(tunables) if tunables is not None else None)
        if not h:
            return False
        self._h = h
        self.imageSize = self._lib.musica_get_image_size(h)
        self.pyramidLevels = self._lib.musica_get_levels(h)
        self.batch = self._lib.musica_get_batch(h)
        return True

    def execute(self, imageData):
        """bool execute(const uint16_t* imageData) — src/vk_processing.cpp:2104-2601 (synchronous)."""
        px = self._pixels(imageData)
        return self._lib.musica_execute(self._h, px.ctypes.data_as(_U16P)) == 1

    def saveOutImage(self, filePath, image_index=0):
        """bool saveOutImage(std::string filePath) — src/vk_processing.cpp:2603-2645."""
        return self._lib.musica_save_out_image(self._h, image_index, os.fsencode(filePath)) == 1

    def debugProcess(self, directory=".", image_index=0):
        """bool debugProcess() — src/vk_processing.cpp:2661-2809 (the reference writes into the cwd)."""
        return self._lib.musica_debug_process(self._h, image_index, os.fsencode(directory)) == 1

    def render_noise_hist(self, image_index=0):
        """noise_hist_render.comp on the cnr level's histogram (RENDER_HISTS, src/vk_processing.cpp:1260-1266, :2347): uint8 [128, 512, 4]."""
        out = np.empty((HIST_RENDER_HEIGHT, HIST_RENDER_WIDTH, 4), dtype=np.uint8)
        self._ok(self._lib.musica_render_noise_hist(self._h, image_index, out.ctypes.data_as(_U8P)), "musica_render_noise_hist")
        return out

    def render_grad_hist(self, image_index=0):
        """gradation_curve_debug_render.comp on the gradation histogram + tone curve (src/vk_processing.cpp:1668-1675, :2508)."""
        out = np.empty((HIST_RENDER_HEIGHT, HIST_RENDER_WIDTH, 4), dtype=np.uint8)
        self._ok(self._lib.musica_render_grad_hist(self._h, image_index, out.ctypes.data_as(_U8P)), "musica_render_grad_hist")
        return out

    def cleanup(self):
        """bool cleanup() — src/vk_processing.cpp:2647-2651."""
        if self._h:
            if self._owned:
                self._lib.musica_destroy(self._h)
            self._h = None
        return True

    def getImageSize(self):
        return self.imageSize

    # ---- extension surface ------------------------------------------------------------
    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    def _pixels(self, imageData):
        px = np.ascontiguousarray(imageData, dtype=np.uint16)
        need = self.batch * self.imageSize * self.imageSize
        if px.size != need:
            raise ValueError("expected %d pixels (batch %d x %d x %d), got %d" % (need, self.batch, self.imageSize, self.imageSize, px.size))
        return px

    def _ok(self, rc, what):
        if rc != 1:
            raise RuntimeError("%s failed: %s" % (what, last_error()))

    def level_size(self, level):
        return self._lib.musica_get_level_size(self._h, level)

    def upload(self, imageData):
        px = self._pixels(imageData)
        self._ok(self._lib.musica_upload(self._h, px.ctypes.data_as(_U16P)), "musica_upload")

    def input_device_ptr(self):
        return self._lib.musica_input_device_ptr(self._h)

    def execute_device(self, d_pixels=None):
        """Enqueue the pipeline on input already resident in HBM (default: the uploaded buffer)."""
        ptr = d_pixels if d_pixels is not None else self.input_device_ptr()
        return self._lib.musica_execute_device(self._h, ptr) == 1

    def sync(self):
        self._ok(self._lib.musica_sync(self._h), "musica_sync")

    def host_alloc(self, shape, dtype=np.uint16):
        """A numpy array in page-locked host memory (inputs of execute_stream move at the PCIe rate from it). Free with host_free()."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self._lib.musica_host_alloc(self._h, n)
        if not p:
            raise MemoryError(last_error())
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).view(dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self._lib.musica_host_free(self._h, p)

    def execute_stream(self, batches, want_stats=False):
        """Pipelined execute over a list of (batch, N, N) uint16 arrays: H2D of batch j + 1 under the kernels of batch j.
        Returns True / False, or (ok, [Stats per image of the sequence]) with want_stats."""
        arrs = [self._pixels(b) for b in batches]
        ptrs = (_VP * len(arrs))(*[a.ctypes.data for a in arrs])
        st = (Stats * (len(arrs) * self.batch))() if want_stats else None
        ok = self._lib.musica_execute_stream(self._h, ptrs, len(arrs), st) == 1
        return (ok, list(st)) if want_stats else ok

    def graded(self):
        n = self.imageSize
        out = np.empty((self.batch, n, n), dtype=np.float32)
        self._ok(self._lib.musica_get_graded(self._h, _f32p(out)), "musica_get_graded")
        return out

    def out_pixels(self, image_index=0):
        n = self.imageSize - 2 * OUT_MARGIN
        out = np.empty((n, n), dtype=np.uint8)
        self._ok(self._lib.musica_get_out_pixels(self._h, image_index, out.ctypes.data_as(_U8P)), "musica_get_out_pixels")
        return out

    def image(self, kind, level=0, image_index=0):
        s = self._lib.musica_image_side(self._h, kind, level)
        if s == 0:
            raise KeyError("no image kind=%d level=%d" % (kind, level))
        out = np.empty((s, s), dtype=np.float32)
        self._ok(self._lib.musica_get_image(self._h, image_index, kind, level, _f32p(out)), "musica_get_image")
        return out

    def set_image(self, kind, level, arr, image_index=0):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        self._ok(self._lib.musica_debug_set_image(self._h, image_index, kind, level, _f32p(a)), "musica_debug_set_image")

    def run_stage(self, stage):
        self._ok(self._lib.musica_debug_run_stage(self._h, stage), "musica_debug_run_stage")

    def noise_hist(self, level, image_index=0):
        out = np.empty(NOISE_BINS, dtype=np.uint32)
        self._ok(self._lib.musica_get_noise_hist(self._h, image_index, level, out.ctypes.data_as(_U32P)), "musica_get_noise_hist")
        return out

    def grad_hist(self, image_index=0):
        out = np.empty(GRAD_BINS, dtype=np.uint32)
        self._ok(self._lib.musica_get_grad_hist(self._h, image_index, out.ctypes.data_as(_U32P)), "musica_get_grad_hist")
        return out

    def noise_hist_max(self, level, image_index=0):
        p = HistMaxPoint()
        self._ok(self._lib.musica_get_noise_hist_max(self._h, image_index, level, C.byref(p)), "musica_get_noise_hist_max")
        return (p.maxValue, p.maxBin)

    def grad_hist_max(self, image_index=0):
        p = HistMaxPoint()
        self._ok(self._lib.musica_get_grad_hist_max(self._h, image_index, C.byref(p)), "musica_get_grad_hist_max")
        return (p.maxValue, p.maxBin)

    def contrast_curve(self, level, image_index=0):
        c = ContrastCurve()
        self._ok(self._lib.musica_get_contrast_curve(self._h, image_index, level, C.byref(c)), "musica_get_contrast_curve")
        return c.as_array()

    def grad_curve(self, image_index=0):
        c = GradCurve()
        self._ok(self._lib.musica_get_grad_curve(self._h, image_index, C.byref(c)), "musica_get_grad_curve")
        return c.as_array(), (c.t0, c.ta, c.t1)

    def tunables(self):
        t = Tunables()
        self._ok(self._lib.musica_get_tunables(self._h, C.byref(t)), "musica_get_tunables")
        return t

    def contrast_params(self, level):
        p = ContrastParams()
        self._ok(self._lib.musica_get_contrast_params(self._h, level, C.byref(p)), "musica_get_contrast_params")
        return (p.lowContrastFactor, p.highContrastFactor)

    def nr_params(self, level):
        p = NrParams()
        self._ok(self._lib.musica_get_nr_params(self._h, level, C.byref(p)), "musica_get_nr_params")
        return (p.lowCnr, p.lowFactor, p.highCnr, p.highFactor)

    def minmax(self, image_index=0):
        a, b = C.c_float(), C.c_float()
        self._ok(self._lib.musica_get_minmax(self._h, image_index, C.byref(a), C.byref(b)), "musica_get_minmax")
        return a.value, b.value

    def stats(self, image_index=0):
        s = Stats()
        self._ok(self._lib.musica_get_stats(self._h, image_index, C.byref(s)), "musica_get_stats")
        return s

    def stats_device(self, d_dst, image_id_base=0, image_id_stride=1):
        """Write batch x musica_stats into caller-owned device memory (async on the ctx stream);
        image_id = image_id_base + index * image_id_stride."""
        self._ok(self._lib.musica_stats_device_strided(self._h, d_dst, image_id_base, image_id_stride), "musica_stats_device")

    def clahe_hist(self, image_index=0):
        out = np.empty((4, 4, 256), dtype=np.uint32)
        self._ok(self._lib.musica_get_clahe_hist(self._h, image_index, out.ctypes.data_as(_U32P)), "musica_get_clahe_hist")
        return out

    def clahe_curves(self, image_index=0):
        out = np.empty((4, 4, 256, 2), dtype=np.float32)
        self._ok(self._lib.musica_get_clahe_curves(self._h, image_index, C.cast(out.ctypes.data, C.POINTER(Point))), "musica_get_clahe_curves")
        return out

    def dispatch(self):
        """(streams, graph): 1 / 2 streams and whether steps replay a captured hipGraph (musica_get_dispatch)."""
        st, g = C.c_int(0), C.c_int(0)
        self._lib.musica_get_dispatch(self._h, C.byref(st), C.byref(g))
        return st.value, bool(g.value)

    def dispatch_text(self):
        st, g = self.dispatch()
        text = "%s, %s" % ({1: "one stream", 2: "two streams (analysis beside the reduce tail)"}[st],
                             "hipGraph replay" if g else "eager launches")
        if self.fuses_noise_hist():
            text += ", level-0 noise histogram inside reduce + band"
        return text

    def fuses_gradhist(self):
        """True when the level-0 expand kernel also accumulates the gradation histogram (no separate k_grad_hist launch)."""
        return self._lib.musica_fuses_gradation_histogram(self._h) == 1

    def fuses_sdev(self):
        """True when the expand launches of levels 0 .. 2 compute sdev themselves and the sdev launches of those levels store nothing."""
        return self._lib.musica_fuses_sdev(self._h) == 1

    def fuses_noise_hist(self):
        """True when level 0's reduce + band launch also counts the level's noise histogram (the level-0 sdev pass is the seam columns only)."""
        return self._lib.musica_fuses_noise_hist(self._h) == 1

    def paired_levels(self):
        """How many k_rb_sdev launches (the sdev pass of level i paired with reduce + band of level i + 1) one whole step runs; 0: no pair."""
        return self._lib.musica_get_paired_levels(self._h)

    def fuses_reduce_band(self):
        """True when level 0's reduce and band kernels are one launch (profile family `reduce_l0` covers both)."""
        return self._lib.musica_fuses_reduce_band(self._h) == 1

    # ---- device-resident output and stream ordering (musica_export_out, musica_stream_*) ---------
    def export_out(self, d_dst, first=0, count=None, fmt=OUT_U8, row_pitch=0, image_pitch=0):
        """Images first .. first + count - 1 (default: the rest of the batch) of the last step into caller-owned device memory at d_dst,
        enqueued on the context's stream. Pitches in bytes; 0: dense (a row's bytes, rows x row_pitch)."""
        count = self.batch - int(first) if count is None else int(count)
        rows, width = out_geometry(self.imageSize, fmt)
        row_pitch = int(row_pitch) or width
        image_pitch = int(image_pitch) or row_pitch * rows
        self._ok(self._lib.musica_export_out(self._h, int(first), count, int(fmt), d_dst, row_pitch, image_pitch), "musica_export_out")

    def stream_wait(self, stream=None):
        """What the context enqueues from now on starts after the work already on `stream` (a hipStream_t handle; None / 0: the null stream)."""
        self._ok(self._lib.musica_stream_wait(self._h, stream or None), "musica_stream_wait")

    def stream_signal(self, stream=None):
        """Work enqueued on `stream` from now on starts after everything enqueued on the context so far."""
        self._ok(self._lib.musica_stream_signal(self._h, stream or None), "musica_stream_signal")

    # ---- similarity metrics of the metamorphic study (musica_sim_*) ---------------------------
    def sim_capture(self, slot, image_index=0):
        """The current 8-bit output of `image_index` into reference slot `slot` (on the device)."""
        self._ok(self._lib.musica_sim_capture(self._h, int(slot), int(image_index)), "musica_sim_capture")

    def sim_set_reference(self, slot, pixels):
        """(N - 20, N - 20) uint8 into reference slot `slot`."""
        n = self.imageSize - 2 * OUT_MARGIN
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        if a.shape != (n, n):
            raise ValueError("expected a %d x %d uint8 plane, got %r" % (n, n, a.shape))
        self._ok(self._lib.musica_sim_set_reference(self._h, int(slot), a.ctypes.data_as(_U8P)), "musica_sim_set_reference")

    def sim_set_vendor_reference(self, slot, pixels):
        """The vendor-processed image ((N - 20, N - 20) uint16 or uint8, the values its DICOM file stores) into reference slot `slot`,
        converted on the device as harness.vendor_to_u8 converts it; 16 or 8 bits from the array's dtype."""
        n = self.imageSize - 2 * OUT_MARGIN
        a = np.asarray(pixels)
        if a.dtype not in (np.uint16, np.uint8) or a.shape != (n, n):
            raise ValueError("expected a %d x %d uint16 or uint8 plane, got %r %s" % (n, n, a.shape, a.dtype))
        a = np.ascontiguousarray(a)
        self._ok(self._lib.musica_sim_set_vendor_reference(self._h, int(slot), a.ctypes.data_as(_VP), 8 * a.itemsize),
                 "musica_sim_set_vendor_reference")

    def sim_compare(self, queries):
        """queries: (image_index, slot, ax, ay, bx, by, w, h) tuples (or SimQuery), all in one launch. Returns one dict per query:
        harness.similarities()' five numbers plus the exact sq_diff_sum, pixels, bins_a / bins_b (== np.histogram(..., bins=256)[0])
        and the min / max of each side."""
        qs = _queries(queries)
        arr, res = (SimQuery * max(len(qs), 1))(*qs), (SimResult * max(len(qs), 1))()
        self._ok(self._lib.musica_sim_compare(self._h, len(qs), arr, res), "musica_sim_compare")
        return [res[i].as_dict() for i in range(len(qs))]

    def sim_rotate_reference(self, dst_slot, src_slot, degree):
        """Reference slot `src_slot` rotated like harness.rotated_reference(slot, degree) into `dst_slot`, on the device."""
        m, off = rotation_params(self.imageSize - 2 * OUT_MARGIN, degree)
        mm, oo = (C.c_double * 4)(*[float(v) for v in m.ravel()]), (C.c_double * 2)(*[float(v) for v in off])
        self._ok(self._lib.musica_sim_rotate_reference(self._h, int(dst_slot), int(src_slot), mm, oo), "musica_sim_rotate_reference")

    def sim_transform_reference(self, dst_slot, src_slot, element):
        """Reference slot `src_slot` as harness.apply_symmetry(slot, element) (element 0 .. 7 of the square's symmetries) into `dst_slot`,
        on the device."""
        if int(element) < 0:
            raise ValueError("symmetry element %d is not in 0 .. 7" % element)
        self._ok(self._lib.musica_sim_transform_reference(self._h, int(dst_slot), int(src_slot), int(element)), "musica_sim_transform_reference")

    def sim_blur_reference(self, dst_slot, src_slot, radius):
        """Reference slot `src_slot` as harness.binomial_blur(slot, radius) (radius 1 .. BLUR_MAX_RADIUS) into `dst_slot`, on the device."""
        if int(radius) < 0:
            raise ValueError("blur radius %d is not in 1 .. %d" % (radius, BLUR_MAX_RADIUS))
        self._ok(self._lib.musica_sim_blur_reference(self._h, int(dst_slot), int(src_slot), int(radius)), "musica_sim_blur_reference")

    def sim_codec_reference(self, dst_slot, src_slot, table, origin=OUT_MARGIN % 8):
        """Reference slot `src_slot` as metrics.block_codec(slot, table, (origin, origin)) (table: codec_table_words; origin 0 .. 7) into
        `dst_slot`, on the device. The default origin is the margin mod 8: the blocks of the raw plane, seen from the output plane."""
        t = codec_table_words(table)
        if not 0 <= int(origin) <= 7:
            raise ValueError("codec origin %d is not in 0 .. 7" % origin)
        self._ok(self._lib.musica_sim_codec_reference(self._h, int(dst_slot), int(src_slot), t.ctypes.data_as(C.POINTER(C.c_uint16)), int(origin)),
                 "musica_sim_codec_reference")

    def sim_zoom_reference(self, dst_slot, src_slot, zoom):
        """Reference slot `src_slot` as harness.zoom(slot, zoom) (zoom = (p, q): zoom_ratio) into `dst_slot`, on the device."""
        p, q = zoom_ratio(zoom)
        self._ok(self._lib.musica_sim_zoom_reference(self._h, int(dst_slot), int(src_slot), p, q), "musica_sim_zoom_reference")

    def sim_scatter_reference(self, dst_slot, src_slot, spec):
        """Reference slot `src_slot` as harness.scatter(slot, spec) (spec = (R, a, b): scatter_spec) into `dst_slot`, on the device."""
        r, a, b = scatter_spec(spec)
        self._ok(self._lib.musica_sim_scatter_reference(self._h, int(dst_slot), int(src_slot), r, a, b), "musica_sim_scatter_reference")

    def sim_warp_reference(self, dst_slot, src_slot, field, origin=OUT_MARGIN):
        """Reference slot `src_slot` as harness.warp(slot, field, (origin, origin)) (field: warp_field) into `dst_slot`, on the device.
        The default origin is the margin: the field of the raw plane, applied to the output plane."""
        f = warp_field(field, self.imageSize - 2 * OUT_MARGIN, origin)
        self._ok(self._lib.musica_sim_warp_reference(self._h, int(dst_slot), int(src_slot), f.ctypes.data_as(C.POINTER(C.c_int16)), f.shape[0], int(origin)),
                 "musica_sim_warp_reference")

    def sim_details(self, details, slot, image_index=0):
        """harness.detail_statistics(output of `image_index`, reference slot `slot`, details) on the device: the details (x, y, r, c) in
        the (N - 20)^2 output plane's coordinates (detail_list; c is not looked at). Returns one dict per detail: "disc" and "ring", each
        the Python ints n, sum_a, sum_b, sum_aa, sum_bb, sum_ab, and box_ssd, box_pixels."""
        ds = detail_list(details, self.imageSize - 2 * OUT_MARGIN, with_contrast=False)
        arr, res = (Detail * len(ds))(*[Detail(*d) for d in ds]), (SimDetailResult * len(ds))()
        self._ok(self._lib.musica_sim_details(self._h, int(image_index), int(slot), len(ds), arr, res), "musica_sim_details")
        return [res[i].as_dict() for i in range(len(ds))]

    def sim_edges(self, edges, slot, image_index=0):
        """harness.edge_statistics(output of `image_index`, reference slot `slot`, edges) on the device: the edges (x, y, h, p, q, o, c)
        in the (N - 20)^2 output plane's coordinates (edge_list; c is not looked at). Returns one dict per edge: the Python ints h, p, q,
        bins, roi_ssd, roi_pixels and the uint32 arrays n, sum_a, sum_b, sum_aa of `bins` entries."""
        es = edge_list(edges, self.imageSize - 2 * OUT_MARGIN, with_contrast=False)
        bins = [edge_bins(e[2], e[3], e[4]) for e in es]
        words = 4 * sum(bins)
        arr, res, tables = (Edge * len(es))(*[Edge(*e) for e in es]), (SimEdgeResult * len(es))(), np.zeros(words, dtype=np.uint32)
        self._ok(self._lib.musica_sim_edges(self._h, int(image_index), int(slot), len(es), arr, res, tables.ctypes.data_as(_U32P), words),
                 "musica_sim_edges")
        return [dict({"h": e[2], "p": e[3], "q": e[4], "bins": bins}, **d) for e, (bins, d) in zip(es, _unpack_tables(res, tables, EDGE_SUMS))]

    def sim_gratings(self, gratings, slot, image_index=0):
        """harness.grating_statistics(output of `image_index`, reference slot `slot`, gratings) on the device: the gratings
        (x, y, h, ux, uy, T, wave) in the (N - 20)^2 output plane's coordinates (grating_list; the wave is not looked at). Returns one
        dict per grating: the Python ints h, ux, uy, T, roi_ssd, roi_pixels and the uint32 arrays n, sum_a, sum_b, sum_aa of T entries."""
        gs = grating_list(gratings, self.imageSize - 2 * OUT_MARGIN, with_wave=False)
        words = 4 * sum(g[5] for g in gs)
        arr, res, tables = (Grating * len(gs))(*[Grating(*g[:6]) for g in gs]), (SimGratingResult * len(gs))(), np.zeros(words, dtype=np.uint32)
        self._ok(self._lib.musica_sim_gratings(self._h, int(image_index), int(slot), len(gs), arr, res, tables.ctypes.data_as(_U32P), words),
                 "musica_sim_gratings")
        return [dict({"h": g[2], "ux": g[3], "uy": g[4], "T": bins}, **d) for g, (bins, d) in zip(gs, _unpack_tables(res, tables, GRATING_SUMS))]

    def sim_points(self, points, slot, groups=None, image_index=0):
        """harness.point_statistics(output of `image_index`, reference slot `slot`, points, groups) on the device: the points
        (x, y, R, s, c, group) in the (N - 20)^2 output plane's coordinates (point_list; c is not looked at), `groups` (default: 1 + the
        largest group) in 1 .. POINT_MAX_GROUPS. Returns {"points": one dict of the Python ints POINT_SUMS per point, "groups": one dict
        per group: "count" and the (S, S) int64 arrays sum_a, sum_b and ssd (POINT_STACKS), indexed [dy + R, dx + R]}."""
        ps = point_list(points, self.imageSize - 2 * OUT_MARGIN, with_contrast=False)
        groups = point_groups(ps, groups)
        side = 2 * ps[0][2] + 1
        words = groups * 3 * side * side
        arr, res, tables = (Defect * len(ps))(*[Defect(*p) for p in ps]), (SimPointResult * len(ps))(), np.zeros(words, dtype=np.uint32)
        self._ok(self._lib.musica_sim_points(self._h, int(image_index), int(slot), len(ps), arr, groups, res, tables.ctypes.data_as(_U32P), words),
                 "musica_sim_points")
        stacks = tables.reshape(groups, 3, side, side).astype(np.int64)
        return {"points": [r.as_dict() for r in res],
                "groups": [dict({"count": sum(1 for p in ps if p[5] == g)}, **{k: stacks[g, i] for i, k in enumerate(POINT_STACKS)}) for g in range(groups)]}

    def sim_observer(self, views, banks, slot, image_index=0):
        """metrics.channel_responses(output of `image_index`, reference slot `slot`, views, banks) on the device: the views (x, y, bank)
        in the (N - 20)^2 output plane's coordinates and the int8 banks (C, S, S) (view_list: ValueError before any call). Returns one
        dict per view: "a" and "b", the int32 arrays of its bank's C channel responses on either side, and the Python ints "pixels"
        (S^2), "sum_a" and "sum_b" (the window's plain sums)."""
        vs, bs = view_list(views, banks, self.imageSize - 2 * OUT_MARGIN)
        words = sum(2 * bs[k].shape[0] for _, _, k in vs)
        barr = (ChannelBank * len(bs))(*[ChannelBank(b.shape[1] // 2, b.shape[0], b.ctypes.data_as(C.POINTER(C.c_int8))) for b in bs])
        arr, res, tables = (View * len(vs))(*[View(*v) for v in vs]), (SimObserverResult * len(vs))(), np.zeros(words, dtype=np.int32)
        self._ok(self._lib.musica_sim_observer(self._h, int(image_index), int(slot), len(bs), barr, len(vs), arr, res,
                                               tables.ctypes.data_as(C.POINTER(C.c_int32)), words), "musica_sim_observer")
        out = []
        for (_, _, k), r in zip(vs, res):
            at, c = int(r.table_offset), bs[k].shape[0]
            out.append({"a": tables[at:at + c].copy(), "b": tables[at + c:at + 2 * c].copy(), "pixels": int(r.pixels), "sum_a": int(r.sum_a), "sum_b": int(r.sum_b)})
        return out

    def _sim_tables(self, name, qs, result_type, dtype, words, *lead, most=None, window=False, trail=()):
        """What sim_profiles / _levels / _gradients / _order / _lattice / _blobs / _spectrum / _cooccurrence / _granulometry / _contours / _minkowski / _reach share: the refusals of sim_<name> before any call
        (most: 1 .. most queries, None: any number; window: sides of 7 at least), its arrays and the call of musica_sim_<name> with `lead`
        in front of the count and `trail` (blobs: the label plane and its length) behind the tables' length. Returns the results and the
        flat tables, `words` zeroed words of `dtype`."""
        if most is not None and not 1 <= len(qs) <= most:
            raise ValueError("sim_%s takes 1 .. %d queries, got %d" % (name, most, len(qs)))
        for i, q in enumerate(qs if window else ()):
            if q.w < 7 or q.h < 7:
                raise ValueError("sim_%s: query %d: region %d x %d is smaller than 7 x 7" % (name, i, q.w, q.h))
        arr, res, tables = (SimQuery * max(len(qs), 1))(*qs), (result_type * max(len(qs), 1))(), np.zeros(max(words, 1), dtype=dtype)
        call = getattr(self._lib, "musica_sim_" + name)
        self._ok(call(self._h, *lead, len(qs), arr, res, tables.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), words, *trail), "musica_sim_" + name)
        return res, tables

    def sim_profiles(self, queries):
        """harness.profile_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, at most PROFILE_MAX_QUERIES, all in one launch. Returns one dict per query: "cols", a (w, 4) uint32
        array, and "rows", (h, 4): per line the exact sum_a, sum_b, sum_dd = sum of (a - b)^2 and sum_aa (PROFILE_SUMS) over the line's
        pixels inside the region; and the Python ints "ssd" (the sum of either table's sum_dd) and "pixels"."""
        qs = _queries(queries)
        res, tables = self._sim_tables("profiles", qs, SimProfileResult, np.uint32, sum(4 * (int(q.w) + int(q.h)) for q in qs))
        out = []
        for r in res[:len(qs)]:
            at, w, h = int(r.table_offset), int(r.cols), int(r.rows)
            out.append({"cols": tables[at:at + 4 * w].reshape(w, 4).copy(), "rows": tables[at + 4 * w:at + 4 * (w + h)].reshape(h, 4).copy(),
                        "ssd": int(r.ssd), "pixels": int(r.pixels)})
        return out

    def sim_levels(self, queries, shift):
        """harness.level_statistics on the device, the classes being the alteration source (alter_set_source) under side a's pixels
        >> shift: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or SimQuery) with w, h >= 1, 1 ..
        LEVEL_MAX_QUERIES of them, all in one launch; shift an integer in LEVEL_MIN_SHIFT .. LEVEL_MAX_SHIFT (ValueError before any call).
        Returns one dict per query: "table", a (classes, 6) uint64 array of the exact n, sum_a, sum_b, sum_dd = sum of (a - b)^2, sum_aa
        and sum_bb (LEVEL_SUMS) per class, and the Python ints "classes", "ssd" (the sum of sum_dd) and "pixels"."""
        classes = level_count(shift)
        qs = _queries(queries)
        res, tables = self._sim_tables("levels", qs, SimLevelResult, np.uint64, len(qs) * classes * len(LEVEL_SUMS), int(shift), most=LEVEL_MAX_QUERIES)
        out = []
        for r in res:
            at, c = int(r.table_offset), int(r.classes)
            out.append({"table": tables[at:at + c * len(LEVEL_SUMS)].reshape(c, len(LEVEL_SUMS)).copy(), "classes": c, "ssd": int(r.ssd), "pixels": int(r.pixels)})
        return out

    def sim_gradients(self, queries):
        """metrics.gradient_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 7, 1 .. SIM_MAX_QUERIES of them, all in one launch (ValueError before any call for a count or a side out
        of range). Returns one dict per query: "table", a (GRADIENT_CLASSES, 6) uint64 array of the exact n, sum_A, sum_B, sum_dot,
        sum_cross (both signed, two's complement) and neg (GRADIENT_FIELDS) per class of the reference side's edge strength, "gsim", the
        mean of q over the interior, and the Python int "pixels" = (w - 2) (h - 2)."""
        qs = _queries(queries)
        per = GRADIENT_CLASSES * len(GRADIENT_FIELDS)
        res, tables = self._sim_tables("gradients", qs, SimGradientResult, np.uint64, len(qs) * per, most=SIM_MAX_QUERIES, window=True)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(GRADIENT_CLASSES, len(GRADIENT_FIELDS)).copy(), "gsim": float(r.gsim), "pixels": int(r.pixels)})
        return out

    def sim_order(self, queries):
        """metrics.order_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 7, 1 .. SIM_MAX_QUERIES of them, all in one launch (ValueError before any call for a count or a side out
        of range). Returns one dict per query: "rings", a (ORDER_RINGS, 5) uint64 array of the exact pairs, same, reversed, flattened
        and split (ORDER_FIELDS) per ring of the 7 x 7 neighbourhood, "histogram", the (ORDER_BINS,) uint64 numbers of interior pixels
        at each census distance 0 .. 96, and the Python int "pixels" = (w - 6) (h - 6)."""
        qs = _queries(queries)
        head = ORDER_RINGS * len(ORDER_FIELDS)
        res, tables = self._sim_tables("order", qs, SimOrderResult, np.uint64, len(qs) * ORDER_TABLE_WORDS, most=SIM_MAX_QUERIES, window=True)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"rings": tables[at:at + head].reshape(ORDER_RINGS, len(ORDER_FIELDS)).copy(),
                        "histogram": tables[at + head:at + ORDER_TABLE_WORDS].copy(), "pixels": int(r.pixels)})
        return out

    def sim_lattice(self, queries, period, origin=0):
        """metrics.lattice_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 2, 1 .. LATTICE_MAX_QUERIES of them, all in one launch; period one of 2, 4, 8, 16, 32 and origin below it
        (lattice_period: ValueError before any call, as for a count or a side out of range). Returns one dict per query: "table", a
        (P, P, 8) uint64 array of the exact LATTICE_FIELDS per [row phase][column phase], and the Python int "pixels" = (w - 1) (h - 1)."""
        P, o = lattice_period(period, origin)
        qs = _queries(queries)
        for i, q in enumerate(qs):
            if q.w < 2 or q.h < 2:
                raise ValueError("sim_lattice: query %d: region %d x %d is smaller than 2 x 2" % (i, q.w, q.h))
        per = P * P * len(LATTICE_FIELDS)
        res, tables = self._sim_tables("lattice", qs, SimLatticeResult, np.uint64, len(qs) * per, P, o, most=LATTICE_MAX_QUERIES)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(P, P, len(LATTICE_FIELDS)).copy(), "pixels": int(r.pixels)})
        return out

    def sim_blobs(self, queries, threshold, connectivity=8, labels=False):
        """metrics.blob_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or SimQuery)
        with w, h >= 1, 1 .. BLOBS_MAX_QUERIES of them, all in one call; threshold 0 .. 254 (blob_threshold) and connectivity 4 or 8
        (ValueError before any call, as for a count out of range). Returns one dict per query, the same as blob_statistics': "table", a
        (BLOB_CLASSES, 6) uint64 array of the exact BLOB_FIELDS per class, the Python ints "pixels", "changed" and "components", the dict
        "largest" (n, first, x0, y0, x1, y1, sum_dd) and, with labels=True, "labels", the (h, w) uint32 plane of the canonical labels."""
        t = blob_threshold(threshold)
        if connectivity not in (4, 8):
            raise ValueError("connectivity %r is neither 4 nor 8" % (connectivity,))
        qs = _queries(queries)
        per = BLOB_CLASSES * len(BLOB_FIELDS)
        planes = np.zeros(sum(int(q.w) * int(q.h) for q in qs), dtype=np.uint32) if labels else None
        res, tables = self._sim_tables("blobs", qs, SimBlobsResult, np.uint64, len(qs) * per, t, int(connectivity), most=BLOBS_MAX_QUERIES,
                                       trail=(planes.ctypes.data_as(_U32P), len(planes)) if labels else (None, 0))
        out = []
        for q, r in zip(qs, res):
            at = int(r.table_offset)
            d = {"table": tables[at:at + per].reshape(BLOB_CLASSES, len(BLOB_FIELDS)).copy(), "pixels": int(r.pixels), "changed": int(r.changed),
                 "components": int(r.components),
                 "largest": {"n": int(r.largest_n), "first": int(r.largest_first), "x0": int(r.largest_x0), "y0": int(r.largest_y0), "x1": int(r.largest_x1),
                             "y1": int(r.largest_y1), "sum_dd": int(r.largest_sum_dd)}}
            if labels:
                lo = int(r.label_offset)
                d["labels"] = planes[lo:lo + int(q.w) * int(q.h)].reshape(int(q.h), int(q.w)).copy()
            out.append(d)
        return out

    def sim_spectrum(self, queries, tile):
        """metrics.spectrum_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, 1 .. SPECTRUM_MAX_QUERIES of them, all in one launch; tile one of 8, 16, 32, 64 (spectrum_tile:
        ValueError before any call, as for a count out of range). Returns one dict per query: "table", a (T, T, 3) int64 array of the
        exact SPECTRUM_FIELDS per [row sequency][column sequency], and the Python int "tiles" = (w // T) (h // T)."""
        T = spectrum_tile(tile)
        qs = _queries(queries)
        per = T * T * len(SPECTRUM_FIELDS)
        res, tables = self._sim_tables("spectrum", qs, SimSpectrumResult, np.int64, len(qs) * per, T, most=SPECTRUM_MAX_QUERIES)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(T, T, len(SPECTRUM_FIELDS)).copy(), "tiles": int(r.tiles)})
        return out

    def sim_cooccurrence(self, queries, levels, distances):
        """metrics.cooccurrence_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, 1 .. COOCCURRENCE_MAX_QUERIES of them, all in one launch; levels one of 8, 16, 32, 64
        (cooccurrence_levels) and distances 1 .. 4 distinct ascending integers 1 .. 16 (cooccurrence_distances): ValueError before any
        call, as for a count out of range. Returns one dict per query: "table", a (D, 4, 2, G, G) uint32 array
        [distance][direction 0, 45, 90, 135][side a = 0, b = 1][level of the first pixel][level of the second], and "pairs", the
        (D, 4) uint64 array of the pairs of every distance and direction."""
        G, ds = cooccurrence_levels(levels), cooccurrence_distances(distances)
        qs = _queries(queries)
        per = len(ds) * 4 * 2 * G * G
        res, tables = self._sim_tables("cooccurrence", qs, SimCooccurrenceResult, np.uint32, len(qs) * per, G, len(ds), (C.c_uint32 * len(ds))(*ds),
                                       most=COOCCURRENCE_MAX_QUERIES)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(len(ds), 4, 2, G, G).copy(),
                        "pairs": np.array([[int(r.pairs[k][i]) for i in range(4)] for k in range(len(ds))], dtype=np.uint64)})
        return out

    def sim_granulometry(self, queries, radii):
        """metrics.granulometry_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, 1 .. GRANULOMETRY_MAX_QUERIES of them, all in one launch; radii 1 .. 8 distinct ascending integers
        1 .. 16 (granulometry_radii): ValueError before any call, as for a count out of range. Returns one dict per query: "table", a
        (K + 1, 2, 5) uint64 array [class, the residue last][polarity bright = 0, dark = 1][sum A, sum B, sum A^2, sum B^2, sum A B],
        and "pixels", w * h."""
        rs = granulometry_radii(radii)
        qs = _queries(queries)
        per = (len(rs) + 1) * 2 * GRANULOMETRY_WORDS
        res, tables = self._sim_tables("granulometry", qs, SimGranulometryResult, np.uint64, len(qs) * per, len(rs), (C.c_uint32 * len(rs))(*rs),
                                       most=GRANULOMETRY_MAX_QUERIES)
        out = []
        for r in res[:len(qs)]:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(len(rs) + 1, 2, GRANULOMETRY_WORDS).copy(), "pixels": int(r.pixels)})
        return out

    def sim_contours(self, queries, threshold, radius, planes=False):
        """metrics.contour_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, 1 .. CONTOURS_MAX_QUERIES of them, all in one call; threshold 1 .. 1 300 500 (contour_threshold) and
        radius 1 .. 32 (contour_radius): ValueError before any call, as for a count out of range. Returns one dict per query, the same
        as contour_statistics': "table", a (2, R^2 + 2) uint64 array [direction a -> b = 0, b -> a = 1][d^2, "far" last], the Python
        ints "contour_a", "contour_b" and "pixels" and, with planes=True, "planes", the (h, w) uint8 plane with bit 0 = a's contour
        and bit 1 = b's."""
        tau, R = contour_threshold(threshold), contour_radius(radius)
        qs = _queries(queries)
        per = 2 * (R * R + 2)
        plane = np.zeros(max(sum(int(q.w) * int(q.h) for q in qs), 1), dtype=np.uint8) if planes else None
        res, tables = self._sim_tables("contours", qs, SimContoursResult, np.uint64, len(qs) * per, tau, R, most=CONTOURS_MAX_QUERIES,
                                       trail=(plane.ctypes.data_as(C.POINTER(C.c_uint8)), len(plane)) if planes else (None, 0))
        out = []
        for q, r in zip(qs, res):
            at = int(r.table_offset)
            d = {"table": tables[at:at + per].reshape(2, R * R + 2).copy(), "contour_a": int(r.contour_a), "contour_b": int(r.contour_b), "pixels": int(r.pixels)}
            if planes:
                lo = int(r.plane_offset)
                d["planes"] = plane[lo:lo + int(q.w) * int(q.h)].reshape(int(q.h), int(q.w)).copy()
            out.append(d)
        return out

    def sim_minkowski(self, queries):
        """metrics.minkowski_statistics on the device: queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or
        SimQuery) with w, h >= 1, 1 .. MINKOWSKI_MAX_QUERIES of them, all in one call: ValueError before any call for a count out of
        range. Returns one dict per query, the same as minkowski_statistics': "table", a (3, 8, 256) uint32 array
        [side a = 0, b = 1, min(a, b) = 2][kind][value], the number of cells of a kind (the pixels; the pixel edges and corners by the
        maximum of their pixels; the interior ones by the minimum; the outline edges) whose value is v, and the Python int "pixels"."""
        qs = _queries(queries)
        per = MINKOWSKI_SIDES * MINKOWSKI_KINDS * 256
        res, tables = self._sim_tables("minkowski", qs, SimMinkowskiResult, np.uint32, len(qs) * per, most=MINKOWSKI_MAX_QUERIES)
        out = []
        for r in res:
            at = int(r.table_offset)
            out.append({"table": tables[at:at + per].reshape(MINKOWSKI_SIDES, MINKOWSKI_KINDS, 256).copy(), "pixels": int(r.pixels)})
        return out

    def sim_reach(self, queries, radii):
        """metrics.reach_statistics on the device, the classes being metrics.reach_classes(source plane, the input the image's current
        output was computed from, radii): queries as sim_compare's, (image_index, slot, ax, ay, bx, by, w, h) tuples (or SimQuery) with
        w, h >= 1, 1 .. REACH_MAX_QUERIES of them, all of one image_index, all in one call; radii as reach_radii takes them (ValueError
        before any call). Returns one dict per query: "table", a (len(radii) + 1, 6) uint64 array of the exact n, changed, sum_a, sum_b,
        sum_dd = sum of (a - b)^2 and max_d = max |a - b| (REACH_FIELDS) per class, and the Python ints "classes", "ssd" (the sum of
        sum_dd), "pixels" and "seeds" (the changed pixels of the whole N x N input plane)."""
        r = reach_radii(radii)
        qs = _queries(queries)
        words = len(qs) * (len(r) + 1) * len(REACH_FIELDS)
        res, tables = self._sim_tables("reach", qs, SimReachResult, np.uint64, words, len(r), r.ctypes.data_as(_U32P), most=REACH_MAX_QUERIES)
        out = []
        for q in res:
            at, c = int(q.table_offset), int(q.classes)
            out.append({"table": tables[at:at + c * len(REACH_FIELDS)].reshape(c, len(REACH_FIELDS)).copy(), "classes": c, "ssd": int(q.ssd),
                        "pixels": int(q.pixels), "seeds": int(q.seeds)})
        return out

    def sim_reach_classes(self, radii, image_index=0):
        """metrics.reach_classes(source plane, the input image_index's current output was computed from, radii) cropped by the margin:
        an (N - 20, N - 20) uint8 array."""
        r = reach_radii(radii)
        n = self.imageSize - 2 * OUT_MARGIN
        out = np.empty((n, n), dtype=np.uint8)
        self._ok(self._lib.musica_sim_reach_classes(self._h, int(image_index), len(r), r.ctypes.data_as(_U32P), out.ctypes.data_as(_U8P)), "musica_sim_reach_classes")
        return out

    def sim_get_reference(self, slot):
        """Reference slot `slot` as an (N - 20, N - 20) uint8 array."""
        n = self.imageSize - 2 * OUT_MARGIN
        out = np.empty((n, n), dtype=np.uint8)
        self._ok(self._lib.musica_sim_get_reference(self._h, int(slot), out.ctypes.data_as(_U8P)), "musica_sim_get_reference")
        return out

    def sim_joint(self, queries, tables=False):
        """queries as sim_compare's, all in one launch. Returns one dict per query: mi, nmi, corr_ratio, tone_mse (harness.tone_similarities'
        numbers but tone_ssim), the entropies h_a, h_b, h_ab, the exact pixels and sq_diff_sum, tone_lut ((256,) uint8: the least-squares
        remap of the slot's gray levels onto the image's) and, with tables=True, "joint": the (256, 256) uint32 counts, row a, column b
        (== harness.joint_histogram)."""
        qs = _queries(queries)
        arr, res = (SimQuery * max(len(qs), 1))(*qs), (SimJointResult * max(len(qs), 1))()
        joint = np.empty((max(len(qs), 1), 256, 256), dtype=np.uint32) if tables else None
        self._ok(self._lib.musica_sim_joint(self._h, len(qs), arr, res, joint.ctypes.data_as(_U32P) if tables else None), "musica_sim_joint")
        out = [res[i].as_dict() for i in range(len(qs))]
        if tables:
            for i, d in enumerate(out):
                d["joint"] = joint[i]
        return out

    def sim_displace(self, queries, radius, tables=False, tiles=False):
        """queries as sim_compare's, all in one launch: the exact sum of squared differences of every query under every integer shift
        (dx, dy) of its slot within `radius` (1 .. SIM_MAX_RADIUS), == harness.displacement_table. Returns one dict per query: pixels,
        ssd_zero (== sim_compare's sq_diff_sum), ssd_min and its shift dx, dy (smallest value, then smallest dx^2 + dy^2, then smallest dy,
        then smallest dx), tiles_x, tiles_y and tiles_off (the 64 x 64 tiles whose own best shift is not (0, 0)); with tables=True "table":
        the (S, S) uint64 sums, row dy, column dx, S = 2 radius + 1; with tiles=True "tile_tables": the (tiles_y, tiles_x, S, S) uint32 sums
        of the tiles. The slot's window grown by `radius` must lie inside the plane."""
        qs = _queries(queries)
        if not 0 <= int(radius) < 2 ** 32:
            raise ValueError("radius %r is not in 1 .. %d" % (radius, SIM_MAX_RADIUS))
        s = 2 * min(int(radius), SIM_MAX_RADIUS) + 1   # a radius beyond the range is refused by the call: the arrays only have to exist
        arr, res = (SimQuery * max(len(qs), 1))(*qs), (SimDisplaceResult * max(len(qs), 1))()
        table = np.zeros((max(len(qs), 1), s, s), dtype=np.uint64) if tables else None
        tile = None
        if tiles:
            per = [((q.h + SIM_TILE - 1) // SIM_TILE) * ((q.w + SIM_TILE - 1) // SIM_TILE) * s * s for q in qs]
            tile = np.zeros(max(sum(per), 1), dtype=np.uint32)
        self._ok(self._lib.musica_sim_displace(self._h, len(qs), arr, int(radius), res,
                                               table.ctypes.data_as(C.POINTER(C.c_uint64)) if table is not None else None,
                                               tile.ctypes.data_as(_U32P) if tile is not None else None), "musica_sim_displace")
        out = [res[i].as_dict() for i in range(len(qs))]
        first = 0
        for i, d in enumerate(out):
            if tables:
                d["table"] = table[i]
            if tiles:
                d["tile_tables"] = tile[first:first + per[i]].reshape(d["tiles_y"], d["tiles_x"], s, s)
                first += per[i]
        return out

    def sim_multiscale(self, queries, scales):
        """queries as sim_compare's, every one at `scales` (1 .. SIM_MAX_SCALES) scales, in one call: the 7 x 7 SSIM of the 2^s x 2^s
        block sums of both sides, == harness.multiscale_similarities. Returns one dict per query: ms_ssim, scales, pixels, the lists
        ssim, cs, lum, mse (SCALE_METRICS), ssd (exact), plane_w, plane_h of length `scales`, and "raw": those arrays at their full
        length (zero beyond `scales`). min(w, h) >> (scales - 1) must be at least 7."""
        qs = _queries(queries)
        if not 0 <= int(scales) < 2 ** 32:
            raise ValueError("scales %r is not in 1 .. %d" % (scales, SIM_MAX_SCALES))
        arr, res = (SimQuery * max(len(qs), 1))(*qs), (SimScalesResult * max(len(qs), 1))()
        self._ok(self._lib.musica_sim_multiscale(self._h, len(qs), arr, int(scales), res), "musica_sim_multiscale")
        return [res[i].as_dict() for i in range(len(qs))]

    def sim_remap_reference(self, dst_slot, src_slot, lut):
        """Reference slot `src_slot` through the 256-entry uint8 table `lut` (dst = lut[src]) into `dst_slot`, on the device."""
        t = np.ascontiguousarray(lut, dtype=np.uint8)
        if t.shape != (256,):
            raise ValueError("expected a table of 256 uint8 values, got %r" % (t.shape,))
        self._ok(self._lib.musica_sim_remap_reference(self._h, int(dst_slot), int(src_slot), t.ctypes.data_as(_U8P)), "musica_sim_remap_reference")

    # ---- ensemble noise statistics (musica_sim_ensemble_*) --------------------------------------
    def sim_ensemble_reset(self):
        """Zeroes the per-pixel accumulators S1 = sum a, S2 = sum a^2 and the realisation count, on the context's stream."""
        self._ok(self._lib.musica_sim_ensemble_reset(self._h), "musica_sim_ensemble_reset")
        self._cov_tracked = None   # the reset drops sim_ensemble_track's regions

    def sim_ensemble_add(self, first=0, count=None):
        """Adds the current 8-bit outputs of images first .. first + count - 1 (default: the rest of the batch) as that many realisations;
        enqueued on the context's stream, returns without waiting. At most SIM_ENSEMBLE_MAX realisations between two resets."""
        count = self.batch - int(first) if count is None else int(count)
        self._ok(self._lib.musica_sim_ensemble_add(self._h, int(first), count), "musica_sim_ensemble_add")

    def sim_ensemble_result(self, queries, tiles=False):
        """queries as sim_compare's (image_index is checked and not used: side a is the ensemble), all in one launch. Returns one dict per
        query: the doubles ENSEMBLE_METRICS and the exact ENSEMBLE_INTEGERS (== harness.ensemble_statistics); with tiles=True
        "tile_tables": the (tiles_y, tiles_x, 2) uint64 pairs (sum D^2, sum V) of the 64 x 64 tiles."""
        qs = _queries(queries)
        arr, res = (SimQuery * max(len(qs), 1))(*qs), (SimEnsembleResult * max(len(qs), 1))()
        tile = None
        if tiles:
            per = [((q.h + SIM_TILE - 1) // SIM_TILE) * ((q.w + SIM_TILE - 1) // SIM_TILE) * 2 for q in qs]
            tile = np.zeros(max(sum(per), 1), dtype=np.uint64)
        self._ok(self._lib.musica_sim_ensemble_result(self._h, len(qs), arr, res,
                                                      tile.ctypes.data_as(C.POINTER(C.c_uint64)) if tile is not None else None),
                 "musica_sim_ensemble_result")
        out = [res[i].as_dict() for i in range(len(qs))]
        first = 0
        for i, d in enumerate(out):
            if tiles:
                d["tile_tables"] = tile[first:first + per[i]].reshape(d["tiles_y"], d["tiles_x"], 2)
                first += per[i]
        return out

    def sim_ensemble_get(self):
        """(S1, S2, K): the two (N - 20, N - 20) uint32 accumulator planes and the realisations added since the last reset. S1 / K is the
        per-pixel mean image, (K S2 - S1^2) / (K (K - 1)) the per-pixel sample variance."""
        n = self.imageSize - 2 * OUT_MARGIN
        s1, s2, k = np.empty((n, n), dtype=np.uint32), np.empty((n, n), dtype=np.uint32), C.c_uint32()
        self._ok(self._lib.musica_sim_ensemble_get(self._h, s1.ctypes.data_as(_U32P), s2.ctypes.data_as(_U32P), C.byref(k)), "musica_sim_ensemble_get")
        return s1, s2, int(k.value)

    def sim_ensemble_track(self, regions, radius):
        """Declares up to SIM_COV_MAX_REGIONS tracked regions (queries as sim_compare's: ax, ay, w, h are used, the rest is checked) for
        the ensemble now starting, after sim_ensemble_reset and before the first add: every later sim_ensemble_add also accumulates the
        lag products of those regions for the lags dy = 0 .. radius, dx = -radius .. radius. A region grown by `radius` to the left, to
        the right and downwards must lie inside the plane. sim_ensemble_reset drops the tracking."""
        qs = _queries(regions)
        if not 0 <= int(radius) < 2 ** 32:
            raise ValueError("radius %r is not in 1 .. %d" % (radius, SIM_MAX_RADIUS))
        arr = (SimQuery * max(len(qs), 1))(*qs)
        self._ok(self._lib.musica_sim_ensemble_track(self._h, int(radius), len(qs), arr), "musica_sim_ensemble_track")
        self._cov_tracked = (qs, int(radius))

    def sim_ensemble_covariance(self, tables=True, tiles=False):
        """One dict per tracked region, in order: the doubles COV_METRICS and the exact COV_INTEGERS (== harness.ensemble_covariance);
        with tables=True "table": the (radius + 1, 2 radius + 1) int64 values C(d) = K P(d) - U(d), row dy, column dx + radius; with
        tiles=True "tile_tables": the (tiles_y, tiles_x, radius + 1, 2 radius + 1) int64 tables of the 64 x 64 tiles. Synchronous;
        changes nothing and may be called again after more adds."""
        qs, radius = getattr(self, "_cov_tracked", None) or ([], 1)
        rows, s = radius + 1, 2 * radius + 1
        res = (SimCovResult * SIM_COV_MAX_REGIONS)()
        table = np.zeros((SIM_COV_MAX_REGIONS, rows, s), dtype=np.int64) if tables else None
        tile = None
        if tiles:
            per = [((q.h + SIM_TILE - 1) // SIM_TILE) * ((q.w + SIM_TILE - 1) // SIM_TILE) * rows * s for q in qs]
            tile = np.zeros(max(sum(per), 1), dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self._ok(self._lib.musica_sim_ensemble_covariance(self._h, res, table.ctypes.data_as(i64p) if table is not None else None,
                                                          tile.ctypes.data_as(i64p) if tile is not None else None), "musica_sim_ensemble_covariance")
        out = [res[i].as_dict() for i in range(len(qs))]
        first = 0
        for i, d in enumerate(out):
            if tables:
                d["table"] = table[i]
            if tiles:
                d["tile_tables"] = tile[first:first + per[i]].reshape(d["tiles_y"], d["tiles_x"], rows, s)
                first += per[i]
        return out

    # ---- alterations of the metamorphic study (musica_alter_*) ---------------------------------
    # Each alter_* writes image `image_index` of the resident input buffer (follow it with execute_device()); the arguments mirror
    # harness.py's generators. Noise kinds draw from Philox4x32-10 keyed by the seed, counter (pixel, block, stream, 0): the same distribution as numpy's, not its stream.
    def alter_set_source(self, raw):
        """One (N, N) uint16 image into the source plane every alteration reads."""
        n = self.imageSize
        a = np.ascontiguousarray(raw, dtype=np.uint16)
        if a.shape != (n, n):
            raise ValueError("expected a %d x %d uint16 image, got %r" % (n, n, a.shape))
        self._ok(self._lib.musica_alter_set_source(self._h, a.ctypes.data_as(_U16P)), "musica_alter_set_source")

    def alter(self, spec, image_index=0):
        self._ok(self._lib.musica_alter(self._h, int(image_index), C.byref(spec)), "musica_alter")

    def alter_none(self, image_index=0):
        self.alter(Alteration(kind=ALTER_NONE), image_index)

    def alter_translate(self, dx, dy=0, image_index=0):
        """harness.clamp_translation(src, dx, dy)."""
        self.alter(Alteration(kind=ALTER_TRANSLATE, dx=int(dx), dy=int(dy)), image_index)

    @staticmethod
    def rotate_spec(side, degree):
        """The Alteration of harness.clamp_rotate(src, degree) for a side x side image."""
        margin = min(100, side // 8)
        m, off = rotation_params(side - 2 * margin, degree)
        return Alteration(kind=ALTER_ROTATE, margin=margin, matrix=(C.c_double * 4)(*[float(v) for v in m.ravel()]),
                          offset=(C.c_double * 2)(*[float(v) for v in off]))

    def alter_rotate(self, degree, image_index=0):
        """harness.clamp_rotate(src, degree)."""
        self.alter(self.rotate_spec(self.imageSize, degree), image_index)

    def alter_symmetry(self, element, image_index=0):
        """harness.apply_symmetry(src, element): np.rot90(src if element < 4 else src.T, element & 3), element 0 .. 7."""
        self.alter(Alteration(kind=ALTER_SYMMETRY, dx=int(element)), image_index)

    def alter_blur(self, radius, image_index=0):
        """harness.binomial_blur(src, radius): the exact binomial blur with weights C(2 radius, k), radius 1 .. BLUR_MAX_RADIUS."""
        if int(radius) < 0:
            raise ValueError("blur radius %d is not in 1 .. %d" % (radius, BLUR_MAX_RADIUS))
        self._ok(self._lib.musica_alter_blur(self._h, int(image_index), int(radius)), "musica_alter_blur")

    def alter_codec(self, table, image_index=0):
        """metrics.block_codec(src, table): the exact 8 x 8 integer block codec with the quantiser table `table` (codec_table_words)."""
        t = codec_table_words(table)
        self._ok(self._lib.musica_alter_codec(self._h, int(image_index), t.ctypes.data_as(C.POINTER(C.c_uint16))), "musica_alter_codec")

    def alter_zoom(self, zoom, image_index=0):
        """harness.zoom(src, zoom): the exact bilinear magnification by p / q about the centre, zoom = (p, q) (zoom_ratio)."""
        p, q = zoom_ratio(zoom)
        self._ok(self._lib.musica_alter_zoom(self._h, int(image_index), p, q), "musica_alter_zoom")

    def alter_scatter(self, spec, image_index=0):
        """harness.scatter(src, spec): the source mixed with its tent x tent blur of box radius R at the scatter fraction a / b,
        spec = (R, a, b) (scatter_spec)."""
        r, a, b = scatter_spec(spec)
        self._ok(self._lib.musica_alter_scatter(self._h, int(image_index), r, a, b), "musica_alter_scatter")

    def alter_details(self, details, image_index=0):
        """harness.insert_details(src, details): the source with the discs (x, y, r, c) of a contrast-detail list (detail_list) inserted."""
        ds = detail_list(details, self.imageSize)
        arr = (Detail * len(ds))(*[Detail(*d) for d in ds])
        self._ok(self._lib.musica_alter_details(self._h, int(image_index), len(ds), arr), "musica_alter_details")

    def alter_edges(self, edges, image_index=0):
        """harness.insert_edges(src, edges): the source with the slanted-edge plates (x, y, h, p, q, o, c) of an edge list (edge_list)
        inserted."""
        es = edge_list(edges, self.imageSize)
        arr = (Edge * len(es))(*[Edge(*e) for e in es])
        self._ok(self._lib.musica_alter_edges(self._h, int(image_index), len(es), arr), "musica_alter_edges")

    def alter_gratings(self, gratings, image_index=0):
        """harness.insert_gratings(src, gratings): the source with the plates (x, y, h, ux, uy, T, wave) of a grating list
        (grating_list) inserted."""
        gs = grating_list(gratings, self.imageSize)
        arr = (Grating * len(gs))(*[Grating(*g[:6]) for g in gs])
        waves = np.array([w for g in gs for w in g[6]], dtype=np.int16)
        self._ok(self._lib.musica_alter_gratings(self._h, int(image_index), len(gs), arr, waves.ctypes.data_as(C.POINTER(C.c_int16)), waves.size),
                 "musica_alter_gratings")

    def alter_points(self, points, image_index=0):
        """harness.insert_points(src, points): the source with the clusters (x, y, R, s, c, group) of a point list (point_list) altered."""
        ps = point_list(points, self.imageSize)
        arr = (Defect * len(ps))(*[Defect(*p) for p in ps])
        self._ok(self._lib.musica_alter_points(self._h, int(image_index), len(ps), arr), "musica_alter_points")

    def alter_warp(self, field, image_index=0):
        """harness.warp(src, field): the exact backward warp by the displacement field on the 64-pixel control grid (warp_field)."""
        f = warp_field(field, self.imageSize)
        self._ok(self._lib.musica_alter_warp(self._h, int(image_index), f.ctypes.data_as(C.POINTER(C.c_int16)), f.shape[0]), "musica_alter_warp")

    def alter_gain(self, gx, gy, image_index=0):
        """harness.apply_gain(src, gx, gy): the source under the separable gain map gx[x] gy[y] / GAIN_ONE^2 (gain_tables), one rounding,
        saturating at 65535."""
        gx, gy = gain_tables(gx, gy, self.imageSize)
        self._ok(self._lib.musica_alter_gain(self._h, int(image_index), gx.ctypes.data_as(_U16P), gy.ctypes.data_as(_U16P)), "musica_alter_gain")

    def alter_lut(self, lut, image_index=0):
        """harness.apply_lut(src, lut): the source mapped point-wise through the tone table (lut_table), lut[v] for every pixel v."""
        lut = lut_table(lut)
        self._ok(self._lib.musica_alter_lut(self._h, int(image_index), lut.ctypes.data_as(_U16P)), "musica_alter_lut")

    def alter_collimator(self, shutter_h, shutter_v, seed=0, stream=0, image_index=0):
        """harness.apply_collimator(src, shutter_h, shutter_v)."""
        self.alter(Alteration(kind=ALTER_COLLIMATOR, shutter_h=int(shutter_h), shutter_v=int(shutter_v), seed=int(seed), stream=int(stream)),
                   image_index)

    def alter_gaussian(self, mean, sigma, seed=0, stream=0, image_index=0):
        """harness.add_gaussian_noise(src, mean, sigma)."""
        self.alter(Alteration(kind=ALTER_GAUSSIAN, mean=float(mean), sigma=float(sigma), seed=int(seed), stream=int(stream)), image_index)

    def alter_poisson(self, factor, seed=0, stream=0, image_index=0):
        """harness.apply_quantum_noise(src, factor)."""
        self.alter(Alteration(kind=ALTER_POISSON, factor=float(factor), seed=int(seed), stream=int(stream)), image_index)

    def alter_draws(self, spec):
        """The (N, N) int32 draws of a noise alteration: k (collimator, Poisson) or the truncated Gaussian noise."""
        n = self.imageSize
        out = np.empty((n, n), dtype=np.int32)
        self._ok(self._lib.musica_alter_draws(self._h, C.byref(spec), out.ctypes.data_as(C.POINTER(C.c_int32))), "musica_alter_draws")
        return out

    def alter_percentile(self, x, y, w, h, q):
        """np.percentile(src[y:y + h, x:x + w], q) of the source plane, computed on the device."""
        out = C.c_double()
        self._ok(self._lib.musica_alter_percentile(self._h, int(x), int(y), int(w), int(h), float(q), C.byref(out)), "musica_alter_percentile")
        return out.value

    def input_pixels(self):
        """The resident input buffer (what musica_upload / musica_alter wrote) as a (batch, N, N) uint16 array."""
        n = self.imageSize
        out = np.empty((self.batch, n, n), dtype=np.uint16)
        self._ok(self._lib.musica_memcpy_d2h(self._h, out.ctypes.data, self.input_device_ptr(), out.nbytes), "musica_memcpy_d2h")
        return out

    # ---- profiling ----------------------------------------------------------------------
    def profile_enable(self, which=True):
        """True: every kernel family; False: off; a list of kernel names: only those families."""
        if which is True:
            mask = -1
        elif not which:
            mask = 0
        else:
            mask = 0
            for name in which:
                mask |= 1 << KERNEL_ID[name]
        self._ok(self._lib.musica_profile_enable(self._h, mask), "musica_profile_enable")

    def profile_reset(self):
        self._ok(self._lib.musica_profile_reset(self._h), "musica_profile_reset")

    def profile(self):
        """{kernel name: (mean microseconds, launches)} since the last reset."""
        out = {}
        for name, kid in KERNEL_ID.items():
            us, n = C.c_double(), C.c_uint64()
            self._ok(self._lib.musica_profile_get(self._h, kid, C.byref(us), C.byref(n)), "musica_profile_get")
            out[name] = (us.value, n.value)
        return out

    # ---- the metric kernel on caller-owned device buffers ---------------------------------
    def device_alloc(self, nbytes):
        p = self._lib.musica_device_alloc(self._h, nbytes)
        if not p:
            raise MemoryError(last_error())
        return p

    def device_free(self, ptr):
        self._lib.musica_device_free(self._h, ptr)

    def h2d(self, d_dst, arr):
        a = np.ascontiguousarray(arr)
        self._ok(self._lib.musica_memcpy_h2d(self._h, d_dst, a.ctypes.data, a.nbytes), "musica_memcpy_h2d")

    def d2h(self, arr, d_src):
        self._ok(self._lib.musica_memcpy_d2h(self._h, arr.ctypes.data, d_src, arr.nbytes), "musica_memcpy_d2h")

    def k_reduce_host(self, images):
        """Fused smooth + downsample of a (batch, S, S) f32 array staged through device buffers."""
        a = np.ascontiguousarray(images, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        b, s, _ = a.shape
        pitch, so = (s + 3) & ~3, (s + 1) // 2
        opitch = (so + 3) & ~3
        padded = np.zeros((b, s, pitch), dtype=np.float32)
        padded[:, :, :s] = a
        d_in, d_out = self.device_alloc(padded.nbytes), self.device_alloc(b * so * opitch * 4)
        try:
            self.h2d(d_in, padded)
            self._ok(self._lib.musica_k_reduce(self._h, d_in, s, pitch, d_out, opitch, b), "musica_k_reduce")
            out = np.empty((b, so, opitch), dtype=np.float32)
            self.d2h(out, d_out)
        finally:
            self.device_free(d_in)
            self.device_free(d_out)
        return out[:, :, :so].copy()

    def selftest_exact_math(self):
        """Mismatch counts of the device-side exact shortcuts over every float bit pattern (all must be 0)."""
        out = (C.c_uint64 * 4)()
        self._ok(self._lib.musica_selftest_exact_math(self._h, out), "musica_selftest_exact_math")
        return list(out)

    def k_reduce_timed(self, side, batch=1, iters=50, seed=0):
        """Mean microseconds per launch of the metric kernel on a random side x side image in HBM."""
        pitch, so = (side + 3) & ~3, (side + 1) // 2
        opitch = (so + 3) & ~3
        rng = np.random.default_rng(seed)
        src = rng.random((batch, side, pitch), dtype=np.float32)
        d_in, d_out = self.device_alloc(src.nbytes), self.device_alloc(batch * so * opitch * 4)
        try:
            self.h2d(d_in, src)
            us = C.c_double()
            self._ok(self._lib.musica_k_reduce_timed(self._h, d_in, side, pitch, d_out, opitch, batch, 3, C.byref(us)), "warmup")
            self._ok(self._lib.musica_k_reduce_timed(self._h, d_in, side, pitch, d_out, opitch, batch, iters, C.byref(us)), "musica_k_reduce_timed")
        finally:
            self.device_free(d_in)
            self.device_free(d_out)
        return us.value


    def k_reduce_cold(self, side, nbuf=8, iters=64, copy_ceiling=True, seed=0):
        """Mean microseconds per launch of the metric kernel on side x side f32 images rotating over `nbuf` distinct
        input / output planes (nbuf * 5 * side^2 bytes must exceed the 256 MiB Infinity Cache for an HBM number),
        and of the copy-shaped ceiling kernel timed the same way. Returns (kernel_us, copy_us or None)."""
        so = side // 2
        rng = np.random.default_rng(seed)
        d_in, d_out = self.device_alloc(nbuf * side * side * 4), self.device_alloc(nbuf * so * so * 4)
        try:
            for k in range(nbuf):
                self.h2d(d_in + k * side * side * 4, rng.random((side, side), dtype=np.float32))
            us, cus = C.c_double(), C.c_double()
            for it in (nbuf, iters):    # first pass: warm-up (code object, TLB)
                self._ok(self._lib.musica_k_reduce_timed_rot(self._h, d_in, side, side, d_out, so, nbuf, it, C.byref(us)), "musica_k_reduce_timed_rot")
            if copy_ceiling:
                for it in (nbuf, iters):
                    self._ok(self._lib.musica_k_copy41_timed_rot(self._h, d_in, side, d_out, nbuf, it, C.byref(cus)), "musica_k_copy41_timed_rot")
        finally:
            self.device_free(d_in)
            self.device_free(d_out)
        return us.value, (cus.value if copy_ceiling else None)


class MusicaPipeline:
    """The C ABI's steps-in-flight object (musica_pipeline_*, include/musica.h): `depth` one-stream contexts of one GPU whose
    steps alternate, with the choice of hardware queues made by musica_pipeline_prime() (what bench.py times)."""

    def __init__(self, imageSize, levels=0, batch=1, depth=3, flags=0, device=0):
        self._lib = load_library()
        p = Params(int(imageSize), int(levels), int(batch), int(device), int(flags))
        self._p = self._lib.musica_pipeline_create(C.byref(p), int(depth))
        if not self._p:
            raise RuntimeError("musica_pipeline_create failed: " + last_error())
        self._device = int(device)
        self.depth = int(depth)
        self._pixels = int(batch) * int(imageSize) * int(imageSize)
        self._borrowed = []

    def _ok(self, rc, what):
        if rc != 1:
            raise RuntimeError("%s failed: %s" % (what, last_error()))

    def upload(self, images):
        """The same batch (batch x N x N uint16) into every context's input buffer."""
        px = np.ascontiguousarray(images, dtype=np.uint16)
        if px.size != self._pixels:      # the C side copies batch * N * N pixels whatever it is handed
            raise ValueError("expected %d pixels (batch x N x N), got %d" % (self._pixels, px.size))
        self._ok(self._lib.musica_pipeline_upload(self._p, px.ctypes.data_as(_U16P)), "musica_pipeline_upload")

    def prime(self, calibration_steps=0):
        self._ok(self._lib.musica_pipeline_prime(self._p, int(calibration_steps)), "musica_pipeline_prime")
        for w in self._borrowed:         # prime() destroys the contexts outside the window it keeps: wrappers handed out before it are void
            w._h = None
        self._borrowed = []

    def calibration(self):
        """{first context of the window: ms per step} of the windows prime() timed ({} when there was nothing to choose)."""
        ms = np.zeros(4, dtype=np.float32)
        n = self._lib.musica_pipeline_calibration(self._p, _f32p(ms))
        return {k: float(ms[k]) for k in range(n)}

    def context(self, k):
        h = self._lib.musica_pipeline_context(self._p, int(k))
        if not h:
            raise IndexError(last_error())
        w = MusicaProcessing._borrow(h, self._device)
        self._borrowed.append(w)
        return w

    def step(self, d_pixels=None):
        self._ok(self._lib.musica_pipeline_step(self._p, d_pixels), "musica_pipeline_step")

    def last(self):
        h = self._lib.musica_pipeline_last(self._p)
        if not h:
            raise RuntimeError(last_error())
        return MusicaProcessing._borrow(h, self._device)

    def sync(self):
        self._ok(self._lib.musica_pipeline_sync(self._p), "musica_pipeline_sync")

    def cleanup(self):
        if self._p:
            self._lib.musica_pipeline_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


def read_raw(path, image_size):
    """The raw reader of test/standalone/main.cpp:54-75; None when the file size does not match."""
    out = np.empty((image_size, image_size), dtype=np.uint16)
    ok = load_library().musica_read_raw(os.fsencode(path), image_size, out.ctypes.data_as(_U16P))
    return out if ok == 1 else None


def write_bmp_gray(path, data):
    d = np.ascontiguousarray(data, dtype=np.uint8)
    h, w = d.shape
    return load_library().musica_write_bmp_gray(os.fsencode(path), w, h, d.ctypes.data_as(_U8P)) == 1


def write_bmp_rgba(path, data):
    d = np.ascontiguousarray(data, dtype=np.uint8)
    h, w, c = d.shape
    assert c == 4
    return load_library().musica_write_bmp_rgba(os.fsencode(path), w, h, d.ctypes.data_as(_U8P)) == 1

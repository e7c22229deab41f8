"""What a study leaves on disk: the reference's CSV files (script.py:223-330) and the files of the study's later options, one table
entry each, and the 8-bit BMP maps of the tile tables. harness re-exports every name."""
import collections
import csv
import os

import numpy as np

from . import processing as mp
from .metrics import BLOB_KEYS, CONTOUR_DIRECTIONS, CONTOUR_DIRECTION_KEYS, CONTOUR_KEYS, COOCCURRENCE_FEATURES, GRANULOMETRY_CLASS_KEYS, GRANULOMETRY_KEYS, GRANULOMETRY_POLARITIES, SPECTRUM_BAND_KEYS, SPECTRUM_KEYS, DETAIL_ROW_KEYS, DETAIL_ROW_STATS, EDGE_ROW_KEYS, EDGE_ROW_STATS, GRADIENT_KEYS, GRATING_ROW_KEYS, GRATING_ROW_STATS, LATTICE_AXIS_KEYS, LATTICE_PERIODS, LEVEL_KEYS, MINKOWSKI_CURVES, MINKOWSKI_KEYS, MINKOWSKI_MATCHED_KEYS, MINKOWSKI_SIDES, OBSERVER_CHANNELS, ORDER_KEYS, POINT_CSV_HEADER, POINT_KEYS, PROFILE_AXES, PROFILE_KEYS, REACH_KEYS, SHIFT_KEYS, WARP_TRACKING_KEYS, displacement_maps, ensemble_maps, nps_map, observer_curve, reach_maps

# ---- the CSV files' headers ---------------------------------------------------------------------
CSV_HEADER = ['raw file', 'alteration', 'altered vs unaltered mse', 'altered vs unaltered ssim', 'altered vs unaltered histogram distance',
              'altered vs reference mse', 'altered vs reference ssim', 'altered vs reference histogram distance',
              'normalized altered vs reference mse', 'normalized altered vs reference ssim',
              'normalized altered vs reference histogram distance']

REF_CSV_HEADER = ['raw file', 'mse similarity', 'ssim similarity', 'histogram distance']   # ref_similarities.csv (script.py:285-290)
TONE_CSV_NAMES = ('mutual information', 'normalized mutual information', 'correlation ratio', 'tone-matched mse', 'tone-matched ssim')   # JOINT_METRICS' order

# A row's comparisons, each the stem of its row keys and its label in the files: a comparison metric's files (METRIC_CSVS) take the key
# <stem>_<suffix>; the two vendor groups stand last, the per-row files have them only for studies that have a vendor image
COMPARISON_CSV_GROUPS = (('direct', 'altered vs unaltered'), ('registered', 'registered vs unaltered'),
                         ('reference', 'altered vs reference'), ('registered_reference', 'registered vs reference'))


def _csv_groups(suffix):
    return tuple(('%s_%s' % (stem, suffix), label) for stem, label in COMPARISON_CSV_GROUPS)


TONE_CSV_GROUPS, SCALE_CSV_GROUPS, GRADIENT_CSV_GROUPS, ORDER_CSV_GROUPS, LATTICE_CSV_GROUPS, BLOB_CSV_GROUPS = \
    (_csv_groups(suffix) for suffix in ('tone', 'scales', 'gradient', 'order', 'lattice', 'blobs'))

SHIFT_CSV_NAMES = ('dx', 'dy', 'sub dx', 'sub dy', 'mse at zero', 'mse at best', 'tiles', 'tiles off')   # SHIFT_KEYS' order
SHIFT_CSV_GROUPS = (('direct_shift', 'direct'), ('registered_shift', 'registered'))
SHIFT_CSV_HEADER = ['raw file', 'alteration'] + ['%s %s' % (g, m) for _, g in SHIFT_CSV_GROUPS for m in SHIFT_CSV_NAMES]   # displacement.csv

SCALE_CSV_METRICS = ("ssim", "cs", "mse")   # per scale 0 .. 4, behind ms_ssim and scales

# order_robustness.csv: one line per row and comparison the row has, in COMPARISON_CSV_GROUPS' order; tau_by_ring spread over three columns
ORDER_CSV_HEADER = ['raw file', 'alteration', 'comparison'] + [c for k in ORDER_KEYS for c in (['tau ring %d' % (i + 1) for i in range(mp.ORDER_RINGS)] if k == "tau_by_ring" else [k])]

# lattice_robustness.csv: one line per row and comparison the row has, in this order; per axis the steps, then phase_mse per period
LATTICE_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'period', 'periodic'] + \
                     ['%s %s' % (axis, c) for axis in ("x", "y") for k in LATTICE_AXIS_KEYS
                      for c in (['phase mse %d' % p for p in LATTICE_PERIODS] if k == "phase_mse" else [k.replace('_', ' ')])]

# blob_robustness.csv: one line per row and comparison the row has, in this order; blob_summary's numbers, the largest component's box,
# then the components and the pixels of every class
BLOB_CSV_HEADER = ['raw file', 'alteration', 'comparison'] + [k.replace('_', ' ') for k in BLOB_KEYS] + ['largest x0', 'largest y0', 'largest x1', 'largest y1'] + \
                  ['%s class %d' % (what, c) for what in ('components', 'pixels') for c in range(mp.BLOB_CLASSES)]

# spectrum_robustness.csv: one line per row, comparison the row has and radial band, ascending; the band's numbers, then the totals of
# the comparison, the same on each of its lines
SPECTRUM_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'tile', 'tiles', 'band'] + list(SPECTRUM_BAND_KEYS) + [k.replace('_', ' ') for k in SPECTRUM_KEYS]

# texture_robustness.csv: one line per row, comparison the row has and distance that has a pair, ascending; the distance's numbers, then
# the comparison's largest divergence, the same on each of its lines
TEXTURE_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'levels', 'distance', 'pairs'] + \
                     ['%s %s' % (f, what) for f in COOCCURRENCE_FEATURES + ('anisotropy',) for what in ('a', 'b', 'difference')] + ['divergence', 'largest divergence']

# granulometry_robustness.csv: one line per row, comparison the row has, polarity and class, the residue (the class behind the last
# radius, without an element) last; the class's numbers, then the polarity's, the same on each of its lines
GRANULOMETRY_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'pixels', 'polarity', 'class', 'radius', 'side', 'sum a', 'sum b'] + \
                          [k.replace('_', ' ') for k in GRANULOMETRY_CLASS_KEYS + GRANULOMETRY_KEYS]

# contour_robustness.csv: one line per row, comparison the row has and direction (a_to_b: the output's contour pixels by their distance
# to the reference's; b_to_a: the reference's by their distance to the output's); the direction's numbers, then the comparison's, the
# same on both of its lines
CONTOUR_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'pixels', 'threshold', 'radius', 'direction'] + \
                     [k.replace('_', ' ') for k in CONTOUR_DIRECTION_KEYS + CONTOUR_KEYS]

# minkowski_robustness.csv: one line per row, comparison the row has and matched area fraction k / 8, k = 1 .. 7 (the tone-free
# read-out: either side at the level where its upper set holds that share of the pixels); the comparison's totals the same on its lines
MINKOWSKI_CSV_HEADER = ['raw file', 'alteration', 'comparison', 'pixels'] + [k.replace('_', ' ') for k in MINKOWSKI_MATCHED_KEYS + MINKOWSKI_KEYS]
# <raw>_minkowski_curves.csv: one line per row, comparison the row has, side (a, b, min) and level 1 .. 255
MINKOWSKI_CURVES_CSV_HEADER = ['alteration', 'comparison', 'side', 'level'] + list(MINKOWSKI_CURVES)

ENSEMBLE_CSV_NAMES = (("mean_shift", "mean shift"), ("bias_rms", "bias rms"), ("noise_rms", "noise rms"), ("bias_fraction", "bias fraction"), ("mse", "mse"))
ENSEMBLE_CSV_METRICS = ("mse", "ssim", "histogram intersection", "histogram distance", "histogram bhattacharyya")   # SIM_METRICS' order
ENSEMBLE_CSV_HEADER = ['raw file', 'alteration', 'realisations'] + ['%s %s' % (g, m) for g in ("direct", "registered") for _, m in ENSEMBLE_CSV_NAMES] + \
                      ['per-realisation %s %s' % (m, w) for m in ENSEMBLE_CSV_METRICS for w in ("mean", "std")]   # ensemble.csv

COV_CSV_NAMES = (("noise_var", "noise var"), ("rho_x", "rho x"), ("rho_y", "rho y"), ("corr_area", "correlation area"), ("hf_fraction", "hf fraction"))
DETAIL_CSV_HEADER = ['raw file', 'alteration', 'radius', 'details'] + ['%s %s' % (k, w) for k in DETAIL_ROW_KEYS for w in DETAIL_ROW_STATS] + \
                    ['outside mse']   # contrast_detail.csv
EDGE_CSV_HEADER = ['raw file', 'alteration', 'orientation', 'edges'] + ['%s %s' % (k, w) for k in EDGE_ROW_KEYS for w in EDGE_ROW_STATS] + \
                  ['outside mse']   # edge_response.csv
GRATING_CSV_HEADER = ['raw file', 'alteration', 'period', 'gratings'] + ['%s %s' % (k, w) for k in GRATING_ROW_KEYS for w in GRATING_ROW_STATS] + \
                     ['outside mse']   # grating_response.csv
GAIN_CSV_HEADER = ['raw file', 'alteration', 'axis', 'lines'] + [k.replace('_', ' ') for k in PROFILE_KEYS]   # gain_response.csv
LEVEL_CSV_HEADER = ['raw file', 'alteration'] + [k.replace('_', ' ') for k in LEVEL_KEYS]   # level_response.csv

REACH_CSV_CLASS = ("outer", "n", "rmse", "changed", "shift", "max")   # reach_summary's per-class lists, in reach.csv's order
REACH_CSV_HEADER = ['raw file', 'alteration', 'class', 'outer radius', 'pixels', 'rmse', 'changed share', 'shift', 'max'] + \
                   [k.replace('_', ' ') for k in REACH_KEYS]   # reach.csv
OBSERVER_CSV_KEYS = ("cho", "auc", "npw", "spread")   # observer_summary's scalars, in observer.csv's order; the channels' snr follow
OBSERVER_CSV_HEADER = ['raw file', 'alteration', 'radius', 'details'] + list(OBSERVER_CSV_KEYS) + ['snr channel %d' % j for j in range(OBSERVER_CHANNELS)]   # observer.csv
OBSERVER_CURVE_CSV_HEADER = ['raw file', 'radius', 'level', 'threshold contrast']   # observer_curve.csv
WARP_CSV_HEADER = ['raw file', 'alteration', 'reach', 'peak'] + [k.replace('_', ' ') for k in WARP_TRACKING_KEYS] + ['registered mse', 'registered ssim']   # warp_response.csv


def covariance_csv_header(radius):
    """noise_covariance.csv of a study with covariance=radius: the groups' numbers, then the radial spectrum of the direct group."""
    return ['raw file', 'alteration', 'realisations', 'radius'] + ['%s %s' % (g, m) for g in ("direct", "registered") for _, m in COV_CSV_NAMES] + \
           ['direct nps radius %d' % i for i in range(int(radius) + 1)]


def _row_csv_header(columns, with_reference):
    """The columns of a comparison metric's per-row file: the raw file, the alteration, then `columns` per group of
    COMPARISON_CSV_GROUPS, the two vendor groups only for studies that have a vendor image."""
    return ['raw file', 'alteration'] + ['%s %s' % (g, c) for _, g in COMPARISON_CSV_GROUPS[:4 if with_reference else 2] for c in columns]


def scale_csv_header(with_reference):
    """scale_robustness.csv's columns: per group ms_ssim, scales, then ssim, cs and mse of scales 0 .. 4; the two vendor groups only for
    studies that have a vendor image."""
    return _row_csv_header(['ms-ssim', 'scales'] + ['%s scale %d' % (m, s) for m in SCALE_CSV_METRICS for s in range(mp.SIM_MAX_SCALES)], with_reference)


def _scale_csv_cells(t):
    if t is None:
        return [""] * (2 + len(SCALE_CSV_METRICS) * mp.SIM_MAX_SCALES)
    return [t["ms_ssim"], t["scales"]] + [t[m][s] if s < t["scales"] else "" for m in SCALE_CSV_METRICS for s in range(mp.SIM_MAX_SCALES)]


def gradient_csv_header(with_reference):
    """gradient_robustness.csv's columns: per group the GRADIENT_KEYS gsim, gc, gain, turn, reversed, rmse and compression, then gain_0
    .. gain_21, the gain of every class of the reference side's edge strength; the two vendor groups only for studies that have a
    vendor image."""
    return _row_csv_header(GRADIENT_KEYS + tuple('gain_%d' % k for k in range(mp.GRADIENT_CLASSES)), with_reference)


def _gradient_csv_cells(t):
    if t is None:
        return [""] * (len(GRADIENT_KEYS) + mp.GRADIENT_CLASSES)
    return ["" if v is None else v for v in [t[k] for k in GRADIENT_KEYS] + list(t["gain_by_class"])]


def tone_csv_header(with_reference):
    """tone_robustness.csv's columns: the five JOINT_METRICS per group, the two vendor groups only for studies that have a vendor image."""
    return _row_csv_header(TONE_CSV_NAMES, with_reference)


def normalized_vs_reference(ref, ovd):
    """m_sim_alt's three normalised values (script.py:272-274): ref_mse / ovd_mse, ref_ssim / ovd_ssim and
    (ref_hist - ovd_hist) / (1 - ovd_hist), with ovd the unaltered result vs the vendor image. IEEE f64 division: a zero denominator
    gives inf or nan (the reference would raise ZeroDivisionError and stop the study)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return [float(np.float64(ref["mse"]) / np.float64(ovd["mse"])), float(np.float64(ref["ssim"]) / np.float64(ovd["ssim"])),
                float((np.float64(ref["hist_distance"]) - ovd["hist_distance"]) / (1.0 - np.float64(ovd["hist_distance"])))]


# ---- the tables' parts ----------------------------------------------------------------------------
SIM_CSV_KEYS = ("mse", "ssim", "hist_distance")   # the reference's three similarities


def _cells(d, keys):
    """The cells of an optional dict: its values under `keys`, or as many empty cells."""
    return [""] * len(keys) if d is None else [d[k] for k in keys]


def _write_csv(out_dir, name, header, lines):
    with open(os.path.join(out_dir, name), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(lines)


def _unaltered(r):
    return r["alteration"] == "unaltered"


def _ovd(rows):
    """The study's unaltered result vs the vendor image (the reference's m_sim_ovd), None for a study without one."""
    return next((r.get("reference") for r in rows if _unaltered(r)), None)


def _lines(studies, cells):
    """One CSV line per row of the studies: the raw file, the alteration, then cells(row, the study's _ovd); none where that is None."""
    for raw_name, rows in studies:
        ovd = _ovd(rows)
        for r in rows:
            c = cells(r, ovd)
            if c is not None:
                yield [raw_name, r["alteration"]] + c


def _ref_columns(ref, ovd):
    return [""] * 6 if ovd is None else _cells(ref, SIM_CSV_KEYS) + normalized_vs_reference(ref, ovd)


def _ensemble_cells(e):
    if e is None:
        return None
    return [e["realisations"]] + [c for key in ("direct", "registered") for c in _cells(e[key], [k for k, _ in ENSEMBLE_CSV_NAMES])] + \
           [e["per_realisation"][w][k] for k in mp.SIM_METRICS for w in ("mean", "std")]


def _covariance_cells(e, radius):
    cov = e["covariance"]
    return [e["realisations"], radius] + [c for key in ("direct", "registered") for c in _cells(cov[key], [k for k, _ in COV_CSV_NAMES])] + \
           list(cov["direct"]["nps_radial"])


def _group_lines(studies, key, groups, cells):
    """A patch relation's CSV lines: one per row that has `key` and per (label, group) of groups(the row's value), in their order: the
    raw file, the alteration, the label, then cells(the value, the group)."""
    for raw_name, rows in studies:
        for r in rows:
            d = r.get(key)
            for label, g in (groups(d) if d else ()):
                yield [raw_name, r["alteration"], label] + cells(d, g)


def _comparison_lines(studies, groups, cells, several=False):
    """The lines of a comparison metric's per-comparison file: one per row, the unaltered one included, and comparison that the row
    has, in the groups' order: the raw file, the alteration, the comparison's label, then cells(its value); several: cells(its value)
    is a list of lines' cells, a line each."""
    for raw_name, rows in studies:
        for r in rows:
            for key, label in groups:
                t = r.get(key)
                if t is not None:
                    for line in (cells(t) if several else [cells(t)]):
                        yield [raw_name, r["alteration"], label] + line


def _blank(v):
    return "" if v is None else v


def _order_cells(t):
    """The ORDER_KEYS with tau_by_ring's three entries in a column each."""
    return [c for k in ORDER_KEYS for c in (list(t[k]) if k == "tau_by_ring" else [t[k]])]


def _lattice_cells(t):
    """The period, the periodic share, then per axis the LATTICE_AXIS_KEYS with phase_mse in a column per period of LATTICE_PERIODS
    (empty beyond the study's period, as every value that is None)."""
    return [len(t["table"]), _blank(t["periodic"])] + \
           [c for axis in ("x", "y") for k in LATTICE_AXIS_KEYS
            for c in ([_blank(t[axis][k].get(p)) for p in LATTICE_PERIODS] if k == "phase_mse" else [_blank(t[axis][k])])]


def _blob_cells(t):
    """blob_summary's BLOB_KEYS, the largest component's box (empty where nothing changed, as every value that is None), then the
    components and the pixels per class."""
    return [_blank(t[k]) for k in BLOB_KEYS] + list(t["largest_box"] or [""] * 4) + list(t["class_components"]) + list(t["class_pixels"])


def _spectrum_lines(t):
    """A line per radial band: the tile, the tiles, the band and its SPECTRUM_BAND_KEYS, then the comparison's SPECTRUM_KEYS (an empty
    cell where one is None)."""
    totals = [_blank(t[k]) for k in SPECTRUM_KEYS]
    return [[t["tile"], t["tiles"], r] + [_blank(band[k]) for k in SPECTRUM_BAND_KEYS] + totals for r, band in enumerate(t["radial"])]


def _texture_lines(t):
    """A line per distance that has a pair: the levels, the distance, its pairs, every feature and the anisotropy of side a, of side b
    and their difference, the distance's divergence, then the comparison's largest."""
    return [[t["levels"], e["distance"], e["pairs"]] + [v for f in COOCCURRENCE_FEATURES + ("anisotropy",) for v in (e["a"][f], e["b"][f], e["difference"][f])] +
            [e["divergence"], t["divergence"]] for e in t["distances"] if e is not None]


def _granulometry_lines(t):
    """A line per polarity and class, the residue last (no radius, side or class numbers): the pixels, the polarity, the class, the
    radius and side of the element that removes it, its exact sums of A and B, share, gain, coherence and mse, then the polarity's mean
    sides, their shift, the slope and the residue's shift."""
    lines = []
    for p, polarity in enumerate(GRANULOMETRY_POLARITIES):
        s = t[polarity]
        totals = [_blank(s[k]) for k in GRANULOMETRY_KEYS]
        for k, words in enumerate(t["table"]):
            c = s["classes"][k] if k < len(s["classes"]) else None
            lines.append([t["pixels"], polarity, k, c["radius"] if c else "", c["side"] if c else "", words[p][0], words[p][1]] +
                         [_blank(c[key]) if c else "" for key in GRANULOMETRY_CLASS_KEYS] + totals)
    return lines


def _contour_lines(t):
    """A line per direction: the pixels, the threshold, the radius, the direction, its found and far pixels and the mean, median and
    95th percentile of the distance over the found ones, then the comparison's sizes, densities, ratio, figure of merit, kept, moved,
    lost and spurious shares and Hausdorff distance."""
    totals = [_blank(t[k]) for k in CONTOUR_KEYS]
    return [[t["pixels"], t["threshold"], t["radius"], d] + [_blank(t[d][k]) for k in CONTOUR_DIRECTION_KEYS] + totals for d in CONTOUR_DIRECTIONS]


def _minkowski_lines(t):
    """A line per matched area fraction: the pixels, the fraction, either side's level and its perimeter and Euler characteristics
    there, then the comparison's totals (MINKOWSKI_KEYS)."""
    totals = [_blank(t[k]) for k in MINKOWSKI_KEYS]
    return [[t["pixels"]] + [m[k] for k in MINKOWSKI_MATCHED_KEYS] + totals for m in t["matched"]]


# The files of the comparison metrics (harness.ROW_METRICS), by key suffix: a study that has direct_<suffix> gets the file.
# per "row": one line per row, header(with_reference), then cells(a group's value or None) for every group; per "comparison": one line
# per row and comparison that the row has, the header as it stands, then cells(the value); per "band": the same with a line for each
# entry of cells(the value).
MetricCsv = collections.namedtuple("MetricCsv", "file per header cells")
METRIC_CSVS = {
    "tone": MetricCsv("tone_robustness.csv", "row", tone_csv_header, lambda t: _cells(t, mp.JOINT_METRICS)),
    "scales": MetricCsv("scale_robustness.csv", "row", scale_csv_header, _scale_csv_cells),
    "gradient": MetricCsv("gradient_robustness.csv", "row", gradient_csv_header, _gradient_csv_cells),
    "order": MetricCsv("order_robustness.csv", "comparison", ORDER_CSV_HEADER, _order_cells),
    "lattice": MetricCsv("lattice_robustness.csv", "comparison", LATTICE_CSV_HEADER, _lattice_cells),
    "blobs": MetricCsv("blob_robustness.csv", "comparison", BLOB_CSV_HEADER, _blob_cells),
    "spectrum": MetricCsv("spectrum_robustness.csv", "band", SPECTRUM_CSV_HEADER, _spectrum_lines),
    "texture": MetricCsv("texture_robustness.csv", "band", TEXTURE_CSV_HEADER, _texture_lines),
    "granulometry": MetricCsv("granulometry_robustness.csv", "band", GRANULOMETRY_CSV_HEADER, _granulometry_lines),
    "contours": MetricCsv("contour_robustness.csv", "band", CONTOUR_CSV_HEADER, _contour_lines),
}


# METRIC_CSVS is the ten entries above and ends with the contours: tests/test_contours_restatement.py holds it to that. The report walks
# SCORED_CSVS, the same files with those of the metrics added since appended (harness.SCORED_METRICS). The tests of a new metric hold
# the outer tables by membership and prefix, never by their last element: the next metric's file is appended HERE, without renaming.
SCORED_CSVS = dict(METRIC_CSVS, minkowski=MetricCsv("minkowski_robustness.csv", "band", MINKOWSKI_CSV_HEADER, _minkowski_lines))


def _spread_cells(count, keys, stats):
    return lambda d, g: [g[count]] + [g[k][w] for k in keys for w in stats] + [d["outside_mse"]]


# file name, header, row key, groups, cells of _group_lines: contrast_detail.csv has one line per cd_ row and radius, ascending;
# edge_response.csv one per edge_ row and orientation; grating_response.csv one per grating_ row and period; gain_response.csv one per
# gain row and axis, the columns' profile first; level_response.csv one per lut row, the number of occupied classes in the label's place
RELATION_CSVS = (
    ("contrast_detail.csv", DETAIL_CSV_HEADER, "details", lambda d: d["radii"].items(), _spread_cells("count", DETAIL_ROW_KEYS, DETAIL_ROW_STATS)),
    ("edge_response.csv", EDGE_CSV_HEADER, "edges", lambda d: d["orientations"].items(), _spread_cells("edges", EDGE_ROW_KEYS, EDGE_ROW_STATS)),
    ("grating_response.csv", GRATING_CSV_HEADER, "gratings", lambda d: d["periods"].items(), _spread_cells("gratings", GRATING_ROW_KEYS, GRATING_ROW_STATS)),
    ("gain_response.csv", GAIN_CSV_HEADER, "profiles", lambda d: [(axis, d[axis]) for axis in PROFILE_AXES], lambda d, g: [g["lines"]] + [g[k] for k in PROFILE_KEYS]),
    ("level_response.csv", LEVEL_CSV_HEADER, "levels", lambda d: [(d[LEVEL_KEYS[0]], d)], lambda d, g: [g[k] for k in LEVEL_KEYS[1:]]),
    # reach.csv: one line per row that has a reach and per class, ascending, the summary's numbers the same on each of its lines
    ("reach.csv", REACH_CSV_HEADER, "direct_reach", lambda d: [(k, k) for k in range(len(d["n"]))],
     lambda d, k: ["" if d[c][k] is None else d[c][k] for c in REACH_CSV_CLASS] + ["" if d[c] is None else d[c] for c in REACH_KEYS]),
    # point_response.csv: one line per point_ row and group, in the groups' order, then "all"
    ("point_response.csv", POINT_CSV_HEADER, "points", lambda d: list(enumerate(d["groups"])) + [("all", d["all"])],
     lambda d, g: [g[k] for k in POINT_KEYS] + [d["outside_mse"]]),
    # observer.csv: one line per cd_ row and radius, ascending
    ("observer.csv", OBSERVER_CSV_HEADER, "observer", lambda d: d["radii"].items(),
     lambda d, g: [g["count"]] + ["" if v is None else v for v in [g[k] for k in OBSERVER_CSV_KEYS] + list(g["channel_snr"])]),
)


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

    Studies run with gradients (rows[0] has "direct_gradient") also get gradient_robustness.csv (gradient_csv_header): one line per
    row, the unaltered one included; cells without a comparison, of a gain that has no value and of an empty class are empty.

    Studies run with order (rows[0] has "direct_order") also get order_robustness.csv (ORDER_CSV_HEADER): one line per row, the
    unaltered one included, and comparison that the row has (none for a comparison that is None): the comparison's name, then
    order_summary's ORDER_KEYS, tau_by_ring in three columns.

    Studies run with lattice=P (rows[0] has "direct_lattice") also get lattice_robustness.csv (LATTICE_CSV_HEADER): one line per row,
    the unaltered one included, and comparison that the row has: the comparison's name, the period, the periodic share, then per axis
    step a, step b, amplified and the largest-over-mean per-phase mse of every period up to P.

    Studies run with blobs=T (rows[0] has "direct_blobs") also get blob_robustness.csv (BLOB_CSV_HEADER): one line per row, the
    unaltered one included, and comparison that the row has: the comparison's name, blob_summary's numbers, the largest component's
    box, then the components and the pixels of every size class.

    Studies run with spectrum=T (rows[0] has "direct_spectrum") also get spectrum_robustness.csv (SPECTRUM_CSV_HEADER): one line per
    row, the unaltered one included, comparison that the row has (none where its region holds no whole tile) and radial band 0 .. log2 T:
    the comparison's name, T, the tiles, the band, its gain, coherence and error share, then spectrum_summary's totals of the
    comparison, the same on each of its lines.

    Studies run with texture=G (rows[0] has "direct_texture") also get texture_robustness.csv (TEXTURE_CSV_HEADER): one line per row,
    the unaltered one included, comparison that the row has (none where its region has no pair) and distance that has a pair: the
    comparison's name, G, the distance, its pairs, contrast, dissimilarity, homogeneity, energy, entropy, correlation and anisotropy
    of side a, of side b and their difference, the distance's Jensen-Shannon divergence, then the comparison's largest divergence, the
    same on each of its lines.

    Studies run with granulometry=radii (rows[0] has "direct_granulometry") also get granulometry_robustness.csv
    (GRANULOMETRY_CSV_HEADER): one line per row, the unaltered one included, comparison that the row has, polarity (bright, dark) and
    class, the residue last: the comparison's name, its pixels, the polarity, the class, the radius and side of the element that removes
    it, the exact sums of A and B, the pattern-spectrum shares of either side, gain, coherence and mse (empty for the residue), then
    the polarity's mean element sides, their shift, the slope of log gain on log side and the residue's shift, the same on each of its
    lines.

    Studies run with contours=tau (rows[0] has "direct_contours") also get contour_robustness.csv (CONTOUR_CSV_HEADER): one line per
    row, the unaltered one included, comparison that the row has and direction (a_to_b: the output's contour pixels by their distance
    to the reference's, b_to_a the other way round): the comparison's name, its pixels, the threshold, the radius, the direction, its
    found and far pixels, the mean, median and 95th percentile of the distance over the found ones, then the sizes, densities and ratio
    of the two contours, Pratt's figure of merit, the kept, moved and lost shares of the reference's contour, the spurious share of the
    output's and the Hausdorff distance, the same on both of its lines.

    Studies run with minkowski=True (rows[0] has "direct_minkowski") also get minkowski_robustness.csv (MINKOWSKI_CSV_HEADER): seven
    lines per row, the unaltered one included, and comparison that the row has, one per matched area fraction k / 8: the comparison's
    name, its pixels, the fraction, the level at which either side's upper set holds that share of the pixels and its perimeter and two
    Euler characteristics there, then the comparison's totals (the mean, total variation, islands, holes and outline contact of either
    side, the gain of the total variation, the normalised L1 distances of the curves, the overlap of the upper sets and the two matched
    distances), the same on each of its lines.

    Studies run with ensemble=K (rows[0] has "ensemble") also get ensemble.csv (ENSEMBLE_CSV_HEADER): one line per noise row, K, the
    mean shift, bias rms, noise rms, bias fraction and mse of the direct and of the registered ensemble (empty without one), then the mean
    and standard deviation over the realisations of the five similarity metrics.

    Studies run with covariance=R (their noise rows' "ensemble" has "covariance") also get noise_covariance.csv
    (covariance_csv_header): one line per noise row, K, R, the noise variance, rho x, rho y, correlation area and high-frequency
    fraction of the direct and of the registered region (empty without one), then the radial noise power spectrum of the direct one.

    Studies run with details (rows[0] has "details") also get contrast_detail.csv (DETAIL_CSV_HEADER): one line per cd_ row and radius,
    the number of details of that radius, the mean, min, max and population std over their positions of contrast, cnr, rose and halo,
    and the row's outside mse (the same on each of its lines).

    Studies run with edges (rows[0] has "edges") also get edge_response.csv (EDGE_CSV_HEADER): one line per edge_ row and orientation,
    the number of edges of that orientation, the min, mean, max over them and the count of those that have the number (an empty cell
    where none has) of step, rise, overshoot, undershoot, mtf50 and mtf_peak, and the row's outside mse.

    Studies run with gratings (rows[0] has "gratings") also get grating_response.csv (GRATING_CSV_HEADER): one line per grating_ row
    and period, the number of gratings of that period (one in each direction of the grid that has it), the median, min, max over them
    and the count of those that have the number (an empty cell where none has) of gain, thd and response, and the row's outside mse.

    Studies run with gains (rows[0] has "profiles") also get gain_response.csv (GAIN_CSV_HEADER): one line per gain row and axis
    ("cols": the column profile, scored against gx; "rows": against gy), the number of lines and profile_summary's numbers of the
    axis (an empty cell where one is None).

    Studies run with luts (rows[0] has "levels") also get level_response.csv (LEVEL_CSV_HEADER): one line per lut row, level_summary's
    numbers of the full frame (an empty cell where one is None).

    Studies run with points (rows[0] has "points") also get point_response.csv (POINT_CSV_HEADER): one line per point_ row and group
    (the index of the cluster size), then one for all the row's points ("all"): point_summary's scalars (an empty cell where one is
    None) and the row's outside mse.

    Studies run with reach (rows[0] has "direct_reach") also get reach.csv (REACH_CSV_HEADER): one line per row whose alteration
    changed some but not all input pixels and per distance class, ascending: the class, its outer radius (empty for the open last
    class), its pixels, rmse, changed share, mean shift and max (empty for an empty class), then reach_summary's numbers of the row
    (seeds, classes, last class, extent, floor, spill, half reach, decay; an empty cell where one is None), the same on each line.

    Studies run with observer (rows[0] has "observer") also get observer.csv (OBSERVER_CSV_HEADER): one line per cd_ row and radius,
    ascending: the number of details of that radius, the model observer's cho, auc, npw and spread and the snr of its Laguerre-Gauss
    channels (an empty cell where one is None); and observer_curve.csv (OBSERVER_CURVE_CSV_HEADER): one line per study and radius, the
    contrast at which cho crosses the level 1 (observer_curve; the level is a convention, not a finding), empty where it never does.

    Studies run with warps (rows[0] has "warp") also get warp_response.csv (WARP_CSV_HEADER): one line per warp row, the field's reach
    and peak displacement in pixels, the four tracking numbers of metrics.warp_tracking (empty without a displacement radius) and the
    registered mse and ssim (empty where the row has no registered comparison)."""
    os.makedirs(out_dir, exist_ok=True)
    having = lambda key: [(raw_name, rows) for raw_name, rows in studies if rows and key in rows[0]]   # noqa: E731
    ensembles = having("ensemble")
    covs = [(raw_name, [r for r in rows if r.get("ensemble") and "covariance" in r["ensemble"]]) for raw_name, rows in ensembles]
    covs = [(raw_name, rows) for raw_name, rows in covs if rows]
    radius = covs[0][1][0]["ensemble"]["covariance"]["direct"]["radius"] if covs else 0
    # file name, header, the studies it covers, cells(row, ovd) behind the raw file and the alteration (None: no line for this row)
    tables = [
        ("direct_robustness.csv", CSV_HEADER, studies,
         lambda r, ovd: None if _unaltered(r) else _cells(r["direct"], SIM_CSV_KEYS) + _ref_columns(r.get("reference"), ovd)),
        ("reg_based_robustness.csv", CSV_HEADER, studies,
         lambda r, ovd: None if _unaltered(r) or r["registered"] is None else
         _cells(r["registered"], SIM_CSV_KEYS) + _ref_columns(r.get("registered_reference"), ovd)),
        ("mean_cnr.csv", ["raw file", "alteration", "mean cnr"], studies if mean_cnr else None, lambda r, ovd: [r["mean_cnr"]]),
        ("displacement.csv", SHIFT_CSV_HEADER, having("direct_shift") or None,
         lambda r, ovd: [c for key, _ in SHIFT_CSV_GROUPS for c in _cells(r.get(key), SHIFT_KEYS)]),
        ("ensemble.csv", ENSEMBLE_CSV_HEADER, ensembles or None, lambda r, ovd: _ensemble_cells(r["ensemble"])),
        ("noise_covariance.csv", covariance_csv_header(radius), covs or None, lambda r, ovd: _covariance_cells(r["ensemble"], radius)),
        ("warp_response.csv", WARP_CSV_HEADER, having("warp") or None,
         lambda r, ovd: None if r["warp"] is None else [r["warp"]["reach"], r["warp"]["peak"]] + _cells(r["warp"]["tracking"], WARP_TRACKING_KEYS) +
         _cells(r["registered"], ("mse", "ssim"))),
    ]
    for name, header, covered, cells in tables:
        if covered is not None:
            _write_csv(out_dir, name, header, _lines(covered, cells))
    for suffix, metric in SCORED_CSVS.items():
        covered, groups = having("direct_" + suffix), _csv_groups(suffix)
        if covered and metric.per == "row":
            groups = groups[:4 if any(groups[2][0] in rows[0] for _, rows in covered) else 2]
            _write_csv(out_dir, metric.file, metric.header(len(groups) == 4),
                       _lines(covered, lambda r, ovd: [c for key, _ in groups for c in metric.cells(r.get(key))]))
        elif covered:
            _write_csv(out_dir, metric.file, metric.header, _comparison_lines(covered, groups, metric.cells, metric.per == "band"))
    for name, header, key, groups, cells in RELATION_CSVS:
        if having(key):
            _write_csv(out_dir, name, header, _group_lines(having(key), key, groups, cells))
    if having("observer"):
        _write_csv(out_dir, "observer_curve.csv", OBSERVER_CURVE_CSV_HEADER,
                   [[raw_name, radius, 1.0, "" if c is None else c] for raw_name, rows in having("observer") for radius, c in observer_curve(rows, 1.0).items()])
    ovds = [[raw_name] + _cells(_ovd(rows), SIM_CSV_KEYS) for raw_name, rows in studies if _ovd(rows) is not None]
    if ovds:
        _write_csv(out_dir, "ref_similarities.csv", REF_CSV_HEADER, ovds)


def _write_maps(studies, out_dir, images):
    """images(row): the (name, uint8 image) pairs of a row, none for a row without them. Writes <raw>_<alteration>_<name>.bmp for each and
    returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for raw_name, rows in studies:
        stem = os.path.splitext(os.path.basename(raw_name.replace("\\", "/")))[0]
        for r in rows:
            for what, img in images(r):
                path = os.path.join(out_dir, "%s_%s_%s.bmp" % (stem, r["alteration"], what))
                if not mp.write_bmp_gray(path, img):
                    raise RuntimeError("writing %s failed: %s" % (path, mp.last_error()))
                written.append(path)
    return written


def _ensemble_images(r):
    e = r.get("ensemble")
    if e is None or "tile_tables" not in e["direct"]:
        return ()
    return zip(("bias", "noise"), ensemble_maps(e["direct"]["tile_tables"], *e["direct"]["size"], e["realisations"]))


def _covariance_images(r):
    e = r.get("ensemble")
    g = e["covariance"]["direct"] if e and "covariance" in e else None
    return () if g is None or "table" not in g else (("nps", nps_map(g["table"], g["realisations"], g["pixels"])),)


def _displacement_images(r):
    t = r.get("registered_shift")
    return () if t is None or "tile_tables" not in t else zip(("rmse", "shift"), displacement_maps(t["tile_tables"], *t["size"]))


def _reach_images(r):
    d = r.get("direct_reach")
    return () if d is None or "class_plane" not in d else zip(("reach_classes", "reach_rmse"), reach_maps(d["class_plane"], d["rmse"]))


def write_reach_maps(studies, out_dir):
    """Two 8-bit BMPs per row of studies run with reach_maps that has a reach: <raw>_<alteration>_reach_classes.bmp, the class of every
    output pixel (class 0 white, the last class black), and <raw>_<alteration>_reach_rmse.bmp, the per-class rmse as bars. Returns the
    paths written."""
    return _write_maps(studies, out_dir, _reach_images)


def _contour_images(r):
    d = r.get("registered_contours")
    return () if d is None or "planes" not in d else (("contours", (np.asarray(d["planes"], dtype=np.uint8) & 3) * 85),)


def write_contour_maps(studies, out_dir):
    """One 8-bit BMP per registered row of studies run with contour_maps: <raw>_<alteration>_contours.bmp, the two contours of the
    registered comparison: 85 where only the output has a contour pixel, 170 where only the reference has one, 255 where both have.
    Returns the paths written."""
    return _write_maps(studies, out_dir, _contour_images)


def write_minkowski_curves(studies, out_dir):
    """One CSV per raw file of studies run with minkowski_curves: <raw>_minkowski_curves.csv (MINKOWSKI_CURVES_CSV_HEADER), a line per
    row, comparison that the row has, side (a, b, min) and level 1 .. 255: the area, perimeter, two Euler characteristics and outline
    contact of the side's upper set at that level. Returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for raw_name, rows in studies:
        lines = [[r["alteration"], label, side, t] + [int(v) for v in d["curves"][s, :, t]]
                 for r in rows for key, label in _csv_groups("minkowski") for d in [r.get(key)] if d is not None and "curves" in d
                 for s, side in enumerate(MINKOWSKI_SIDES) for t in range(1, 256)]
        if lines:
            name = "%s_minkowski_curves.csv" % os.path.splitext(os.path.basename(raw_name.replace("\\", "/")))[0]
            _write_csv(out_dir, name, MINKOWSKI_CURVES_CSV_HEADER, lines)
            written.append(os.path.join(out_dir, name))
    return written


def write_ensemble_maps(studies, out_dir):
    """Two 8-bit BMPs per noise row of studies run with ensemble_tiles (ensemble_maps: one pixel per 64 x 64 tile of the full frame):
    <raw>_<alteration>_bias.bmp, the tile's bias rms against the unaltered result, and <raw>_<alteration>_noise.bmp, its noise rms, in
    gray levels. Returns the paths written."""
    return _write_maps(studies, out_dir, _ensemble_images)


def write_covariance_maps(studies, out_dir):
    """One 8-bit BMP per noise row of studies run with covariance_tiles: <raw>_<alteration>_nps.bmp, the centred noise power spectrum of
    the direct region (nps_map: S x S pixels, the zero frequency in the middle, log-scaled). Returns the paths written."""
    return _write_maps(studies, out_dir, _covariance_images)


def write_displacement_maps(studies, out_dir):
    """Two 8-bit BMPs per registered row of studies run with displacement_tiles (displacement_maps: one pixel per 64 x 64 tile):
    <raw>_<alteration>_rmse.bmp, the tile RMSE at the zero shift, and <raw>_<alteration>_shift.bmp, the length of the tile's best shift.
    Returns the paths written."""
    return _write_maps(studies, out_dir, _displacement_images)


def write_study_csvs(rows, out_dir, raw_name, mean_cnr=True):
    """write_studies_csvs for one raw image: direct_robustness.csv / reg_based_robustness.csv with the reference's column layout,
    mean_cnr.csv, and (rows of a study with a vendor image) the "vs reference" columns and ref_similarities.csv."""
    write_studies_csvs([(raw_name, rows)], out_dir, mean_cnr=mean_cnr)

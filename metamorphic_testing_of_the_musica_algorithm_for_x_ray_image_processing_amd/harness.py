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


# ---- running the pipeline -------------------------------------------------------------------------

class Runner:
    """Processes raw images to the 8-bit output the reference's saveOutImage writes (margin cropped)."""

    def __init__(self, image_size, levels=0, device=0, use_cli=False, device_metrics=False, device_alterations=False):
        if use_cli and device_alterations:
            raise ValueError("device alterations write the library's resident input buffer: the CLI path has none")
        if use_cli and device_metrics:
            raise ValueError("device metrics score the library's device output: the CLI path has none")
        self.n, self.levels, self.device, self.use_cli = image_size, levels, device, use_cli
        self.device_alterations = device_alterations   # run_study generates the alterations on the device (musica_alter); implies device_metrics
        self.device_metrics = device_metrics or device_alterations   # run_study scores on the device (musica_sim_compare) instead of with numpy
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

    def close(self):
        if self.proc:
            self.proc.cleanup()


def read_bmp_gray(path):
    """Reads the 24-bpp bottom-up BMP saveOutImage writes; returns the gray channel top-down."""
    b = open(path, "rb").read()
    off = int.from_bytes(b[10:14], "little")
    w, h = int.from_bytes(b[18:22], "little"), int.from_bytes(b[22:26], "little")
    row = (w * 3 + 3) & ~3
    a = np.frombuffer(b, dtype=np.uint8, count=row * h, offset=off).reshape(h, row)[:, 0:w * 3:3]
    return a[::-1].copy()


def run_study(raw, runner, rng=None, shutters=None, translations=None, rotations=None, sigmas=None, factors=None):
    """The reference's per-image loop (script.py:383-657): returns a list of rows
    {alteration, direct: {...}, registered: {...} or None, mean_cnr}. With runner.device_metrics the similarities are computed
    on the device against the unaltered result kept in reference slot 0 (rotations: the rotated unaltered result in slot 1).

    With runner.device_alterations the raw image is uploaded once and every alteration is generated on the device (musica_alter),
    the rotated unaltered result comes from musica_sim_rotate_reference, and the seed of the noise alterations is drawn from `rng`, their
    ordinal in the study being the stream. The geometric alterations are bit-identical to the host's, so their rows equal a device-metrics
    study's; the noise rows (c_sh_*, gn_*, pn_*) come from a different, reproducible, stream than the host study's numpy draws."""
    rng = rng or np.random.default_rng(0)
    n = raw.shape[0]
    shutters = scaled(SHUTTERS, n) if shutters is None else shutters
    translations = scaled(TRANSLATIONS, n) if translations is None else translations
    rotations = ROTATIONS if rotations is None else rotations
    sigmas = GAUSS_SIGMAS if sigmas is None else sigmas
    factors = POISSON_FACTORS if factors is None else factors
    device = getattr(runner, "device_metrics", False)
    alter_on_device = getattr(runner, "device_alterations", False)
    unalt = runner.run(raw)
    shape = unalt.shape
    full = (0, 0, 0, 0, shape[1], shape[0])

    def on_device(queries):
        return [{k: r[k] for k in mp.SIM_METRICS} for r in runner.proc.sim_compare(queries)]

    if device:
        runner.proc.sim_capture(0)
        direct = on_device([(0, 0) + full])[0]
    else:
        direct = similarities(unalt, unalt)
    rows = [{"alteration": "unaltered", "direct": direct, "registered": None, "mean_cnr": runner.mean_cnr() if runner.proc else None}]

    if alter_on_device:
        runner.proc.alter_set_source(raw)
        seed = int(rng.integers(0, 2 ** 63))
        ordinal = [0]

        def dev(make):
            """An alteration as a no-argument call: make(seed, stream) enqueues it on the device, with the study ordinal as stream."""
            ordinal[0] += 1
            k = ordinal[0]
            return lambda: make(seed, k)

    def add(name, altered_raw, reg=None, roi=None):
        """altered_raw: the altered image, or (device alterations) a call that writes it into the resident input buffer.
        reg: the host crop; roi: () -> (region, slot) of the same comparison on the device (region None: no registration)."""
        row = {"alteration": name, "registered": None}
        if callable(altered_raw):
            altered_raw()
            runner.run_resident()
        elif device:
            runner.run_device(altered_raw)
        if device:
            queries = [(0, 0) + full]
            if roi is not None:
                region, slot = roi()
                if region is not None and min(region[4], region[5]) >= 8:
                    queries.append((0, slot) + region)
            res = on_device(queries)
            row["direct"] = res[0]
            if len(res) > 1:
                row["registered"] = res[1]
        else:
            alt = runner.run(altered_raw)
            row["direct"] = similarities(alt, unalt)
            if reg is not None:
                a, u = reg(alt, unalt)
                if a.size and a.shape == u.shape and min(a.shape) >= 8:
                    row["registered"] = similarities(a, u)
        row["mean_cnr"] = runner.mean_cnr() if runner.proc else None
        rows.append({k: row[k] for k in ("alteration", "direct", "registered", "mean_cnr")})

    def rotated_slot(d):
        if alter_on_device:
            runner.proc.sim_rotate_reference(1, 0, d)
        else:
            runner.proc.sim_set_reference(1, rotated_reference(unalt, d))
        return roi_rotation(shape, d), 1

    if alter_on_device:
        p = runner.proc
        for s in shutters:
            add("c_sh_%d" % s, dev(lambda seed, k, s=s: p.alter_collimator(s, s, seed, k)), None, lambda s=s: (roi_collimator(shape, s), 0))
        for t in translations:
            add("t_x_%d" % t, dev(lambda seed, k, t=t: p.alter_translate(t, 0)), None, lambda t=t: (roi_translation_x(shape, t), 0))
        for t in translations:
            add("t_y_%d" % t, dev(lambda seed, k, t=t: p.alter_translate(0, t)), None, lambda t=t: (roi_translation_y(shape, t), 0))
        for d in rotations:
            add("r_%d" % d, dev(lambda seed, k, d=d: p.alter_rotate(d)), None, lambda d=d: rotated_slot(d))
        for sg in sigmas:
            add("gn_%s" % sg, dev(lambda seed, k, sg=sg: p.alter_gaussian(0.0, sg, seed, k)))
        for f in factors:
            add("pn_%s" % f, dev(lambda seed, k, f=f: p.alter_poisson(f, seed, k)))
        return rows

    for s in shutters:
        add("c_sh_%d" % s, apply_collimator(raw, s, s, rng), lambda a, u, s=s: register_collimator(a, u, s),
            lambda s=s: (roi_collimator(shape, s), 0))
    for t in translations:
        add("t_x_%d" % t, clamp_translation(raw, t, 0), lambda a, u, t=t: register_translation_x(a, u, t),
            lambda t=t: (roi_translation_x(shape, t), 0))
    for t in translations:
        add("t_y_%d" % t, clamp_translation(raw, 0, t), lambda a, u, t=t: register_translation_y(a, u, t),
            lambda t=t: (roi_translation_y(shape, t), 0))
    for d in rotations:
        add("r_%d" % d, clamp_rotate(raw, d), lambda a, u, d=d: register_rotation(a, u, d), lambda d=d: rotated_slot(d))
    for sg in sigmas:
        add("gn_%s" % sg, add_gaussian_noise(raw, 0.0, sg, rng))
    for f in factors:
        add("pn_%s" % f, apply_quantum_noise(raw, f, rng))
    return rows


# ---- command line: the reference's three CSV files (script.py:223-330) -------------------------
CSV_HEADER = ['raw file', 'alteration', 'altered vs unaltered mse', 'altered vs unaltered ssim', 'altered vs unaltered histogram distance',
              'altered vs reference mse', 'altered vs reference ssim', 'altered vs reference histogram distance',
              'normalized altered vs reference mse', 'normalized altered vs reference ssim',
              'normalized altered vs reference histogram distance']


def write_study_csvs(rows, out_dir, raw_name, mean_cnr=True):
    """direct_robustness.csv / reg_based_robustness.csv with the reference's column layout. The six "vs reference"
    columns compare with the vendor-processed image, which the reference tree does not ship (missing blobs): they
    stay empty. mean_cnr.csv adds what test/mean_cnr/script.py reports per alteration."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "direct_robustness.csv"), "w", newline="") as fd, \
            open(os.path.join(out_dir, "reg_based_robustness.csv"), "w", newline="") as fr:
        wd, wr = csv.writer(fd), csv.writer(fr)
        wd.writerow(CSV_HEADER)
        wr.writerow(CSV_HEADER)
        for r in rows:
            if r["alteration"] == "unaltered":
                continue
            d = r["direct"]
            wd.writerow([raw_name, r["alteration"], d["mse"], d["ssim"], d["hist_distance"]] + [""] * 6)
            if r["registered"] is not None:
                g = r["registered"]
                wr.writerow([raw_name, r["alteration"], g["mse"], g["ssim"], g["hist_distance"]] + [""] * 6)
    if mean_cnr:
        with open(os.path.join(out_dir, "mean_cnr.csv"), "w", newline="") as fc:
            wc = csv.writer(fc)
            wc.writerow(["raw file", "alteration", "mean cnr"])
            for r in rows:
                wc.writerow([raw_name, r["alteration"], r["mean_cnr"]])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Metamorphic study of one raw image (or a seeded phantom) on the HIP MUSICA path")
    ap.add_argument("--raw", help="raw file: 256-byte header + N*N little-endian uint16 (test/standalone/main.cpp:54-75)")
    ap.add_argument("--phantom-seed", type=int, default=1, help="seed of the synthetic phantom used when --raw is absent")
    ap.add_argument("--size", type=int, default=3072, help="image side N (the reference's CLI fixes 3072)")
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--out", default="out", help="directory of the CSV files")
    ap.add_argument("--cli", action="store_true", help="run every image through the musica-standalone process (run_process, script.py:200-214)")
    ap.add_argument("--device-metrics", action="store_true", help="compute MSE, SSIM and the histogram distances on the GPU (musica_sim_compare)")
    ap.add_argument("--device-alterations", action="store_true",
                    help="generate the alterations on the GPU (musica_alter; implies --device-metrics); the noise rows then come from a "
                         "different, reproducible, random stream than the host study's")
    args = ap.parse_args(argv)
    if args.cli and args.device_alterations:
        ap.error("--device-alterations writes the in-process library's input buffer: it cannot be combined with --cli")
    if args.cli and args.device_metrics:
        ap.error("--device-metrics scores the in-process library's device output: it cannot be combined with --cli")
    if args.raw:
        from .processing import read_raw
        raw = read_raw(args.raw, args.size)
        name = os.path.basename(args.raw)
    else:
        from .phantom import phantom
        raw = phantom(args.size, args.phantom_seed, noise=4.0)
        name = "phantom_%d_seed%d" % (args.size, args.phantom_seed)
    runner = Runner(args.size, args.levels, use_cli=args.cli, device_metrics=args.device_metrics, device_alterations=args.device_alterations)
    rows = run_study(raw, runner, rng=np.random.default_rng(0))
    runner.close()
    write_study_csvs(rows, args.out, name, mean_cnr=not args.cli)
    print("wrote %d alterations to %s" % (len(rows) - 1, args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""One sha256 per row and key of a study with every option on, and one per CSV file that write_studies_csvs makes of it, for comparing
two trees bit for bit: what a change of harness.py or report.py must leave alone. Three paths, each its own study of a seeded phantom:
  * host          a stand-in for the pipeline (a 3 x 3 box mean of the raw image's high bits, cropped by the margin) scored by the host's
                  restatements, at N = 84: no GPU needed;
  * metrics       harness.Runner with device_metrics at N = 151: 131 x 131 outputs, 3 x 3 tiles with a ragged tail;
  * alterations   harness.Runner with device_alterations at N = 151, with ensemble=3 and covariance=2 and their tile tables.
Every study has one value per grid of the reference's alterations, a d4, blur, zoom, scatter, warp and codec row, one grid or spec of
every patch relation with its *_tables flag on and the observer, a vendor image, tone, scales=2, gradients, order, lattice=8, blobs=3,
spectrum=8, texture=8 (distances 1, 3), granulometry=(1, 3), contours=900 (radius 5), minkowski with its curves, reach with its tables and maps, and displacement=2 with its tile tables. An option that the tree's run_study does not have
yet is left out, and --off leaves options out by name: what remains compares with a tree from before them.
Prints one JSON line {path: {"rows": {alteration: {key: sha256}}, "keys": the rows' keys in order, "csv": {file: sha256}}}. Run it on two trees on one machine and
compare the lines; the digests pin nothing from version to version (the ABI does not promise f64 bits), so they are not committed.
  python devtools/study_rows.py [--tree DIR] [--paths host,metrics,alterations] [--off spectrum,texture,texture_distances,granulometry,contours,contour_radius,minkowski,minkowski_curves]   # DIR: the checkout whose package is imported"""
import argparse
import hashlib
import inspect
import json
import os
import struct
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--paths", default="host,metrics,alterations")
ap.add_argument("--off", default="", help="a comma list of run_study's options to leave out")
args = ap.parse_args()
paths = args.paths.split(",")
if not paths or any(p not in ("host", "metrics", "alterations") for p in paths):
    raise SystemExit("study_rows: --paths takes a comma list out of host,metrics,alterations")
sys.path.insert(0, os.path.abspath(args.tree))
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

if set(paths) - {"host"} and mp.device_count() < 1:
    raise SystemExit("study_rows: no HIP device")


def raw(v):
    """The bytes of a row's value: arrays as they lie in memory, floats as IEEE doubles, integers as 64 bits, containers in order (a
    dict by its sorted keys), None and strings marked as such."""
    if v is None:
        return b"\x00none"
    if isinstance(v, str):
        return b"\x00str" + v.encode()
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if isinstance(v, dict):
        return b"".join(str(k).encode() + raw(v[k]) for k in sorted(v, key=str))
    if isinstance(v, (list, tuple)):
        return b"".join(raw(x) for x in v)
    if isinstance(v, (float, np.floating)):
        return struct.pack("<d", v)
    return struct.pack("<q" if v < 0 else "<Q", int(v))


class HostRunner:
    """harness.Runner's interface on the host path: the "processor" is a fixed function of the raw image."""
    device_metrics = device_alterations = False

    def __init__(self, n):
        self.n, self.proc, self.last = n, self, None

    def run(self, image, workdir=None):
        v = (np.asarray(image) >> 4).astype(np.int64)
        box = sum(np.roll(np.roll(v, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) // 9
        b = H.PROCESSING_MARGIN
        self.last = np.clip(box[b:-b, b:-b], 0, 255).astype(np.uint8)
        return self.last

    def mean_cnr(self):
        return float(self.last.mean())

    def close(self):
        pass


def study(path):
    n = 84 if path == "host" else 151
    image = phantom(n, 1, noise=4.0)
    out = n - 2 * H.PROCESSING_MARGIN
    options = dict(
        shutters=[8], translations=[n // 4], rotations=[9], sigmas=[16.0], factors=[0.05],
        vendor=np.random.default_rng(3).integers(0, 65536, size=(out, out)).astype(np.uint16), symmetries=[1], blurs=[2], zooms=[(5, 4)],
        scatters=[H.SCATTERS(n)[0]], warps=H.WARPS(n)[:1], codecs=[64], details=[H.detail_grid(n, 8)], detail_tables=True, observer=True,
        edges=[H.edge_grid(n, 8)], edge_tables=True, gratings=[H.grating_grid(n, 8)], grating_tables=True, gains=H.GAINS(n)[:1], gain_tables=True,
        luts=H.LUTS(image)[:1], lut_tables=True, points=[H.point_grid(n, 64)], point_tables=True, tone=True, scales=2, gradients=True, order=True,
        lattice=8, blobs=3, spectrum=8, texture=8, texture_distances=(1, 3), granulometry=(1, 3), contours=900, contour_radius=5, minkowski=True, minkowski_curves=True, reach=True, reach_tables=True, reach_maps=True, displacement=2, displacement_tiles=True)
    for name in list(options):
        if name not in inspect.signature(H.run_study).parameters or name in args.off.split(","):
            del options[name]
    if path == "alterations":
        options.update(ensemble=3, ensemble_tiles=True, covariance=2, covariance_tiles=True)
    runner = HostRunner(n) if path == "host" else H.Runner(n, device_metrics=path == "metrics", device_alterations=path == "alterations", ensemble_batch=2)
    try:
        rows = H.run_study(image, runner, rng=np.random.default_rng(0), **options)
    finally:
        runner.close()
    digest = {"rows": {r["alteration"]: {k: hashlib.sha256(raw(v)).hexdigest() for k, v in r.items()} for r in rows}, "keys": [list(r) for r in rows], "csv": {}}
    with tempfile.TemporaryDirectory() as d:
        H.write_studies_csvs([("phantom_%d" % n, rows)], d)
        for name in sorted(os.listdir(d)):
            with open(os.path.join(d, name), "rb") as f:
                digest["csv"][name] = hashlib.sha256(f.read()).hexdigest()
    return digest


print(json.dumps({path: study(path) for path in paths}))

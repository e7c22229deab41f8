"""The model-observer relation on the device (kernels_observer.hip) beside its yardsticks, in ONE run on one device, on the default
contrast-detail grid of an image (detail_grid(n, 64): discs of radius 1 .. 32, windows of side 9 .. 133, one Laguerre-Gauss bank of
seven channels per radius): kernel times of musica_sim_observer (k_observer) and of musica_sim_details (k_sim_details, the nearest
existing kernel: one workgroup per detail over the same boxes, 13 unweighted sums) from a `rocprofv3 --kernel-trace` run of this script
in --launch-only mode (a child process), the wall time of the two synchronous calls from the same child, and the wall time of
metrics.channel_responses, the host restatement, on the same planes and grid. Prints one JSON line: per kernel and call the calls,
the median, the least and the largest time in us.

The launches rotate over --contexts contexts (each with its own output and reference slot), one at a time, so that no launch finds its
planes in the 256 MiB Infinity Cache: 8 contexts x 47 MB at 3072^2.
  python devtools/observer_probe.py [--n 3072] [--reps 40] [--contexts 8]
  python devtools/observer_probe.py --launch-only      # what the profiled child runs
  python devtools/observer_probe.py --host-only        # the host restatement alone, on random planes (needs no device)
  PROBE_LIB=<path>/libmusica_hip_NAME.so python devtools/observer_probe.py ...   # another build of the library, as devtools/gain_probe.py"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

KERNELS = ("k_observer", "k_sim_details")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--contexts", type=int, default=8)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--launch-only", action="store_true")
ap.add_argument("--host-only", action="store_true")
args = ap.parse_args()
if os.environ.get("PROBE_LIB"):   # A/B against another build of the library (the profiled child inherits the variable)
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])
n = args.n
nw = n - 2 * mp.OUT_MARGIN
details = H.output_details(H.detail_grid(n, 64))
views, banks = H.observer_views(details)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def host_times(a, b):
    took = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        H.channel_responses(a, b, views, banks)
        took.append((time.perf_counter() - t0) * 1e6)
    return took


def grid_facts():
    sides = [banks[k].shape[1] for _, _, k in views]
    return {"details": len(details), "radii": sorted(set(d[2] for d in details)), "channels": int(banks[0].shape[0]),
            "window_pixels": int(sum(s * s for s in sides)), "pixel_bytes_read": int(sum(5 * s * s for s in sides)),
            "multiply_adds": int(sum(2 * banks[k].shape[0] * banks[k].shape[1] ** 2 for _, _, k in views))}


if args.host_only:
    rng = np.random.default_rng(2)
    planes = [rng.integers(0, 256, (nw, nw), dtype=np.uint8) for _ in range(2)]
    print(json.dumps({"n": n, "grid": grid_facts(), "host": {"channel_responses": summary(host_times(*planes))}}))
    raise SystemExit(0)
if mp.device_count() < 1:
    raise SystemExit("observer_probe: no HIP device")

if args.launch_only:
    raw = phantom(n, 1, noise=4.0)
    ctxs = []
    for _ in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        assert p.execute(raw), mp.last_error()
        p.sim_capture(0)   # the times do not depend on the values: the output against its own capture
        ctxs.append(p)
    walls = {}
    for name, call in (("sim_observer", lambda p: p.sim_observer(views, banks, 0)), ("sim_details", lambda p: p.sim_details(details, 0))):
        took = []
        for k in range(args.reps + args.contexts):   # the first round warms up (and allocates the call's buffers)
            p = ctxs[k % args.contexts]
            p.sync()
            t0 = time.perf_counter()
            call(p)                                   # synchronous: returns behind the stream
            took.append((time.perf_counter() - t0) * 1e6)
        walls[name] = took[args.contexts:]
    walls["channel_responses (host)"] = host_times(ctxs[0].out_pixels(), ctxs[0].sim_get_reference(0))
    for p in ctxs:
        p.cleanup()
    print("WALLS " + json.dumps(walls))
    raise SystemExit(0)


def profiled(cmd, warm):
    """({kernel: [durations in us]}, the child's wall times) of a command under rocprofv3 --kernel-trace; the first `warm` launches
    of each kernel are dropped."""
    d = tempfile.mkdtemp(prefix="observer_probe_")
    try:
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("observer_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        walls = next((json.loads(line[6:]) for line in r.stdout.splitlines() if line.startswith("WALLS ")), {})
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("musica::", "")
            if name in KERNELS:
                times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        for k, v in times.items():
            if len(v) != args.reps + warm:
                raise SystemExit("observer_probe: %d launches of %s, expected %d" % (len(v), k, args.reps + warm))
        return {k: v[warm:] for k, v in times.items()}, walls
    finally:
        shutil.rmtree(d, ignore_errors=True)


if shutil.which("rocprofv3") is None:
    raise SystemExit("observer_probe: rocprofv3 not found")
times, walls = profiled([sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps), "--contexts", str(args.contexts),
                         "--host-reps", str(args.host_reps)], args.contexts)
print(json.dumps({"n": n, "library": os.path.basename(mp.LIB_PATH), "grid": grid_facts(),
                  "kernels": {k: summary(v) for k, v in sorted(times.items())},
                  "calls_under_the_profiler": {k: summary(v) for k, v in sorted(walls.items())}}))

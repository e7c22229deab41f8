"""The local-order metric on the device (kernels_order.hip) beside its yardsticks, in ONE run on one device: kernel times of
musica_sim_order (k_order), of musica_sim_gradients (k_gradients and k_gradients_fold) and of musica_sim_compare (k_sim and k_sim_fold),
which read the same 4 + 1 bytes per pixel, on the same full-frame query, from a `rocprofv3 --kernel-trace` run of this script in
--launch-only mode (a child process), and the wall time of the three synchronous calls from the same child. Three scenes, each a round
of its own:
  phantom    the output of a seeded phantom against the captured output of the same phantom with a quarter of the noise: a radiograph's orders
  identical  the same output against its own capture: every pixel at d = 0, the most contended histogram bin
  random     random bytes on both sides: all 97 bins, every category
Prints one JSON line: per scene and kernel the calls, the median, the least and the largest time in us.

The launches rotate over --contexts contexts (each with its own output and reference slot), one at a time, so that no launch finds its
planes in the 256 MiB Infinity Cache: 16 contexts x 20.7 MB at 2048^2.
  python devtools/order_probe.py [--n 2048] [--reps 40] [--contexts 16]
  python devtools/order_probe.py --launch-only      # what the profiled child runs
  PROBE_LIB=<path>/libmusica_hip_NAME.so python devtools/order_probe.py ...   # another build of the library, as devtools/gain_probe.py"""
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
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

SCENES = ("phantom", "identical", "random")
CALLS = ("sim_order", "sim_gradients", "sim_compare")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2048)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--contexts", type=int, default=16)
ap.add_argument("--launch-only", action="store_true")
args = ap.parse_args()
if os.environ.get("PROBE_LIB"):   # A/B against another build of the library (the profiled child inherits the variable)
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])
if mp.device_count() < 1:
    raise SystemExit("order_probe: no HIP device")
n = args.n
nw = n - 2 * mp.OUT_MARGIN
full = (0, 0, 0, 0, 0, 0, nw, nw)

if args.launch_only:
    rng = np.random.default_rng(2)
    quiet, noisy = phantom(n, 1, noise=1.0), phantom(n, 1, noise=4.0)
    ctxs = []
    for _ in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        ctxs.append(p)
    walls = {}
    for scene in SCENES:
        for p in ctxs:   # slot 0: the scene's reference; the output: the scene's side a
            if scene == "phantom":
                assert p.execute(quiet), mp.last_error()
                p.sim_capture(0)
                assert p.execute(noisy), mp.last_error()
            elif scene == "identical":
                p.sim_capture(0)                          # the noisy phantom's output is still the context's
            else:
                p.set_image(mp.IMG_GRADED, 0, ((rng.integers(0, 256, (n, n)) + 0.5) / 255.0).astype(np.float32))
                p.sim_set_reference(0, rng.integers(0, 256, (nw, nw), dtype=np.uint8))
        for name in CALLS:
            took = []
            for k in range(args.reps + args.contexts):   # the first round warms up (and allocates the call's buffers)
                p = ctxs[k % args.contexts]
                p.sync()
                t0 = time.perf_counter()
                getattr(p, name)([full])                  # synchronous: returns behind the stream
                took.append((time.perf_counter() - t0) * 1e6)
            walls["%s %s" % (scene, name)] = took[args.contexts:]
    for p in ctxs:
        p.cleanup()
    print("WALLS " + json.dumps(walls))
    raise SystemExit(0)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def profiled(cmd, warm):
    """({scene: {kernel: [durations in us]}}, the child's wall times) of a command under rocprofv3 --kernel-trace; the first `warm`
    launches of each round are dropped. A kernel's launches come in len(SCENES) rounds, in the scenes' order."""
    d = tempfile.mkdtemp(prefix="order_probe_")
    try:
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("order_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        walls = next((json.loads(line[6:]) for line in r.stdout.splitlines() if line.startswith("WALLS ")), {})
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("musica::", "")
            if name in ("k_order", "k_gradients", "k_gradients_fold", "k_sim", "k_sim_fold"):
                times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        per = args.reps + warm
        out = {}
        for k, v in times.items():
            if len(v) != per * len(SCENES):
                raise SystemExit("order_probe: %d launches of %s, expected %d" % (len(v), k, per * len(SCENES)))
            for i, scene in enumerate(SCENES):
                out.setdefault(scene, {})[k] = v[i * per + warm:(i + 1) * per]
        return out, walls
    finally:
        shutil.rmtree(d, ignore_errors=True)


if shutil.which("rocprofv3") is None:
    raise SystemExit("order_probe: rocprofv3 not found")
times, walls = profiled([sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps), "--contexts", str(args.contexts)],
                        args.contexts)
print(json.dumps({"n": n, "library": os.path.basename(mp.LIB_PATH), "pixels": nw * nw, "bytes_read": nw * nw * 5,
                  "kernels": {scene: {k: summary(v) for k, v in sorted(ks.items())} for scene, ks in times.items()},
                  "calls_under_the_profiler": {k: summary(v) for k, v in sorted(walls.items())}}))

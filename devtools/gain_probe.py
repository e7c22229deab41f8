"""The gain pair on the device (kernels_gain.hip) beside its yardsticks, in ONE run on one device: kernel times of the gain map
(musica_alter_gain, k_alter_gain, N^2 u16 under gain_vignette's map: both tables vary) and of the plain copy of the same bytes into the
same buffer (k_alter's MUSICA_ALTER_NONE), and of the profiles of the full output frame (musica_sim_profiles: k_sim_profiles and, in the
shipped form, k_sim_profiles_fold) beside the comparison that reads the same bytes (musica_sim_compare: k_sim and k_sim_fold), from a
`rocprofv3 --kernel-trace` run of this script in --launch-only mode (a child process). Then, the profiler off, the same calls between
two device events on a torch stream that the context waits for and signals: what a whole call takes (table upload, launch, and for the
measurements the copy back), which for the gain map is mostly not the kernel. Prints one JSON line.

The launches rotate over --contexts contexts (each with its own source plane, input image and reference slot), one at a time, so that
no launch finds its planes in the 256 MiB Infinity Cache: 12 contexts x 37.7 MB at 3072^2.
  python devtools/gain_probe.py [--n 3072] [--reps 40] [--contexts 12] [--contrast 128] [--stats-out FILE]
  python devtools/gain_probe.py --launch-only      # what the profiled child runs
  PROBE_LIB=<path>/libmusica_hip_NAME.so python devtools/gain_probe.py ...   # another build of the library, as devtools/linear_probe.py:
  bash devtools/build_variant.sh atomics -DMUSICA_PROFILES_ATOMICS gives the other combination form of the profiles"""
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

import numpy as np

if "--launch-only" not in sys.argv:
    import torch  # noqa: E402  (first: libmusica_hip.so then binds to the HIP runtime torch already loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--contexts", type=int, default=12)
ap.add_argument("--contrast", type=int, default=128)
ap.add_argument("--stats-out", help="write the per-kernel statistics (one CSV row per kernel) here")
ap.add_argument("--launch-only", action="store_true")
args = ap.parse_args()
if os.environ.get("PROBE_LIB"):   # A/B against another build of the library (the profiled child inherits the variable)
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])
if mp.device_count() < 1:
    raise SystemExit("gain_probe: no HIP device")
n = args.n
gx, gy = H.gain_vignette(n, args.contrast)
full = (0, 0, 0, 0, 0, 0, n - 2 * mp.OUT_MARGIN, n - 2 * mp.OUT_MARGIN)
CALLS = (("alter_none", lambda p: p.alter_none()), ("alter_gain", lambda p: p.alter_gain(gx, gy)),
         ("sim_compare", lambda p: p.sim_compare([full])), ("sim_profiles", lambda p: p.sim_profiles([full])))


def contexts():
    raw = np.random.default_rng(1).integers(0, 65536, (n, n), dtype=np.uint16)
    plane = np.random.default_rng(2).integers(0, 256, (n - 20, n - 20), dtype=np.uint8)
    ctxs = []
    for _ in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()   # the pyramid is not used: only the source, the input image and the slot
        p.alter_set_source(raw)
        p.sim_set_reference(0, plane)
        ctxs.append(p)
    return ctxs


if args.launch_only:
    ctxs = contexts()
    for _, call in CALLS:
        for k in range(args.reps + args.contexts):   # the first round warms up (and allocates the table buffers)
            p = ctxs[k % args.contexts]
            call(p)
            p.sync()
    for p in ctxs:
        p.cleanup()
    raise SystemExit(0)


def call_times():
    """{call: [us between two device events around the call, launch order]}, the first round over the contexts dropped."""
    stream = torch.cuda.current_stream()
    ctxs = contexts()
    times = {}
    for name, call in CALLS:
        for k in range(args.reps + args.contexts):
            p = ctxs[k % args.contexts]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            p.stream_wait(stream.cuda_stream)
            call(p)
            p.stream_signal(stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            p.sync()
            if k >= args.contexts:
                times.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
    for p in ctxs:
        p.cleanup()
    return times


def kernel_times(cmd, warm):
    """{kernel: [durations in us, launch order]} of a command under rocprofv3 --kernel-trace, the first `warm` launches of each dropped."""
    d = tempfile.mkdtemp(prefix="gain_probe_")
    try:
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("gain_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("musica::", "")
            times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        return {k: v[warm:] for k, v in times.items() if len(v) > warm}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


if shutil.which("rocprofv3") is None:
    raise SystemExit("gain_probe: rocprofv3 not found")
times = kernel_times([sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps),
                      "--contexts", str(args.contexts), "--contrast", str(args.contrast)], args.contexts)
kernels = {k: summary(v) for k, v in sorted(times.items()) if "k_alter" in k or "k_sim" in k}
out = {"n": n, "library": os.path.basename(mp.LIB_PATH), "u16_bytes": n * n * 4, "profile_bytes": (n - 2 * mp.OUT_MARGIN) ** 2 * 5, "kernels": kernels,
       "calls_between_events": {k: summary(v) for k, v in call_times().items()}}
if args.stats_out:
    with open(args.stats_out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["kernel", "calls", "median_us", "min_us", "max_us"])
        for k, s in kernels.items():
            w.writerow([k, s["calls"], s["median_us"], s["min_us"], s["max_us"]])
print(json.dumps(out))

"""The joint-histogram kernel (kernels_joint.hip, musica_sim_joint) beside k_sim (musica_sim_compare) on the same queries: kernel times
from a `rocprofv3 --kernel-trace` run of this script in --launch-only mode (a child process), for one full-frame query of two similar
images ("natural": a processed phantom against the processed phantom with a little more noise), of a flat image against a flat slot (every
lane of a wavefront adds to one LDS address) and of 16 natural queries in one launch; then the wall time of the calls and of a device
study with and without tone=True. Prints one JSON line.

Both entry points are synchronous and the ABI has no event pair around their launches, so the kernel times are the tracer's device
timestamps (start to end of each dispatch), not HIP events; the tracer's own --stats tables are not kept, --stats-out writes the medians.

The launches rotate over --contexts contexts, one at a time, so that no launch finds its planes in the 256 MiB Infinity Cache: 6 contexts
x 46.6 MB (the f32 plane and the u8 slot) at 3072^2.
  python devtools/joint_probe.py [--sizes 2048,3072] [--reps 30] [--contexts 6] [--stats-out FILE] [--no-profile] [--no-study]
  python devtools/joint_probe.py --launch-only --n 3072      # what the profiled child runs
  PROBE_LIB=<pkg>/libmusica_hip_NAME.so python devtools/joint_probe.py ...   # a devtools/build_variant.sh library (-DMUSICA_JOINT_GLOBAL_ATOMICS)"""
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

if os.environ.get("PROBE_LIB"):   # A/B against a library built by devtools/build_variant.sh
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2048,3072")
ap.add_argument("--n", type=int, default=3072, help="--launch-only: the one size to run")
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--contexts", type=int, default=6)
ap.add_argument("--stats-out", help="write the per-case kernel statistics (CSV) here")
ap.add_argument("--study-n", type=int, default=3072)
ap.add_argument("--study-levels", type=int, default=12)
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--no-study", action="store_true")
ap.add_argument("--launch-only", action="store_true")
args = ap.parse_args()
if mp.device_count() < 1:
    raise SystemExit("joint_probe: no HIP device")
CASES = ("natural", "natural_x16", "flat")   # flat last: it overwrites the graded planes


def contexts(n):
    """--contexts contexts holding a processed phantom, with slot 0 = the processed phantom with more noise, slot 1 flat."""
    nw = n - 20
    a, b = phantom(n, 1, noise=4.0), phantom(n, 1, noise=8.0)
    ctxs = []
    for _ in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=args.levels, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        assert p.execute(b), mp.last_error()
        p.sim_capture(0)
        assert p.execute(a), mp.last_error()
        p.sim_set_reference(1, np.full((nw, nw), 90, np.uint8))
        ctxs.append(p)
    return ctxs


def run_cases(n, ctxs, timed=None):
    """Each case: (reps + contexts) rounds of sim_joint then sim_compare on the same queries; the first `contexts` rounds warm up."""
    nw = n - 20
    full = (0, 0, 0, 0, nw, nw)
    flat = np.full((n, n), (120 + 0.5) / 255.0, np.float32)
    for case in CASES:
        if case == "flat":
            for p in ctxs:
                p.set_image(mp.IMG_GRADED, 0, flat)
        queries = [(0, 1 if case == "flat" else 0) + full] * (16 if case == "natural_x16" else 1)
        wall = {"sim_joint": [], "sim_compare": []}
        for r in range(args.reps + args.contexts):
            p = ctxs[r % args.contexts]
            for name, call in (("sim_joint", p.sim_joint), ("sim_compare", p.sim_compare)):
                t0 = time.perf_counter()
                call(queries)
                if r >= args.contexts:
                    wall[name].append((time.perf_counter() - t0) * 1e6)
        if timed is not None:
            timed[case] = {k: round(statistics.median(v), 1) for k, v in wall.items()}


if args.launch_only:
    ctxs = contexts(args.n)
    wall = {}
    run_cases(args.n, ctxs, wall)
    for p in ctxs:
        p.cleanup()
    print(json.dumps({"wall_us": wall}))
    raise SystemExit(0)


def kernel_times(cmd):
    """{kernel: [durations in us, launch order]} of a command under rocprofv3 --kernel-trace, and the command's stdout."""
    d = tempfile.mkdtemp(prefix="joint_probe_")
    try:
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("joint_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("musica::", "")
            times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        return times, r.stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


out = {"lib": os.path.basename(mp.LIB_PATH), "reps": args.reps, "contexts": args.contexts, "sizes": {}}
stats_rows = []
if not args.no_profile:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("joint_probe: rocprofv3 not found")
    per_case = args.reps + args.contexts
    for n in (int(v) for v in args.sizes.split(",")):
        times, stdout = kernel_times([sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--levels", str(args.levels),
                                      "--reps", str(args.reps), "--contexts", str(args.contexts)])
        pixels = (n - 20) ** 2
        entry = {"pixels": pixels, "bound_bytes": 5 * pixels, "wall_us": json.loads(stdout.strip().splitlines()[-1])["wall_us"], "cases": {}}
        for kernel in ("k_joint", "k_sim"):
            v = times.get(kernel, [])                   # the contexts' set-up launches neither; k_sim_fold and k_sim_remap are other names
            assert len(v) == per_case * len(CASES), (kernel, len(v))
            for i, case in enumerate(CASES):
                s = summary(v[i * per_case + args.contexts:(i + 1) * per_case])
                q = 16 if case == "natural_x16" else 1
                s["GBps"] = round(5 * pixels * q / s["median_us"] / 1e3, 1)      # against the joint kernel's bound: 4 B + 1 B per region pixel
                entry["cases"].setdefault(case, {})[kernel] = s
                stats_rows.append([n, case, kernel, s["calls"], s["median_us"], s["min_us"], s["max_us"], s["GBps"]])
        out["sizes"][str(n)] = entry
    if args.stats_out:
        with open(args.stats_out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["n", "case", "kernel", "calls", "median_us", "min_us", "max_us", "GBps_of_5B_per_pixel"])
            w.writerows(stats_rows)

if not args.no_study:
    n = args.study_n
    raw = phantom(n, 1, noise=4.0)
    runner = H.Runner(n, args.study_levels, device_alterations=True)
    runner.run(raw)                                  # warm: code objects, graph capture
    for name, tone in (("study_ms", False), ("study_with_tone_ms", True)):
        H.run_study(raw, runner, rng=np.random.default_rng(0), tone=tone)
        t = []
        for _ in range(4):
            t0 = time.perf_counter()
            rows = H.run_study(raw, runner, rng=np.random.default_rng(0), tone=tone)
            t.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2), "rows": len(rows)}
    runner.close()
print(json.dumps(out))

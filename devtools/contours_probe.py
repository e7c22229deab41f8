"""The contour metric (kernels_contours.hip) on the device beside its yardstick, in ONE run on one device.
  call      musica_sim_contours over the full frame for the (threshold, radius) pairs 4096:16, 4096:32 and 1:16 (or --cases), timed with
            HIP events around the whole synchronous call (a torch stream that the context's stream waits for and signals:
            musica_stream_wait / musica_stream_signal; where torch finds no device, the host's clock around the call, and the output says
            so), beside musica_sim_compare of the same query, which reads the same 4 + 1 bytes a pixel.
  launches  per kernel of the call (k_contour_mask, k_contour_distance) and k_sim / k_sim_fold, from a `rocprofv3 --kernel-trace` run of
            this script in --launch-only mode (a child process); --no-launches leaves that run out.
--content says what the two sides hold:
  random    independent random planes: at threshold 1 the densest contour there is, about three pixels in eight;
  phantom   the processed output of a phantom on side a and the processed output of another one in the slot;
  empty     a random plane on side a and a flat slot: no target anywhere, every walk runs to the radius.
--groups sets MUSICA_CONTOURS_GROUPS, the most workgroups of a query's direction, for the whole run (0: the launcher's own).
Prints one JSON line: per round the events' median time of the call, the two contours' sizes, and per kernel the calls, the median,
the least and the largest time in us.

The calls rotate over --contexts contexts, one at a time, so that no launch finds its planes in the 256 MiB Infinity Cache.
  python devtools/contours_probe.py [--n 3072] [--reps 20] [--contexts 6] [--cases "4096:16;4096:32;1:16"] [--content random] [--groups 0] [--no-launches]
  python devtools/contours_probe.py --launch-only      # what a profiled child runs
  PROBE_LIB=<pkg>/libmusica_hip_NAME.so python devtools/contours_probe.py ...   # a devtools/build_variant.sh library"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--contexts", type=int, default=6)
ap.add_argument("--cases", type=lambda s: tuple((mp.contour_threshold(int(part.split(":")[0])), mp.contour_radius(int(part.split(":")[1]))) for part in s.split(";")),
                default=((4096, 16), (4096, 32), (1, 16)))
ap.add_argument("--content", choices=("random", "phantom", "empty"), default="random")
ap.add_argument("--groups", type=int, default=0)
ap.add_argument("--no-launches", action="store_true")
ap.add_argument("--launch-only", action="store_true")
args = ap.parse_args()
if args.groups:
    os.environ["MUSICA_CONTOURS_GROUPS"] = str(args.groups)   # read at every call
if os.environ.get("PROBE_LIB"):   # A/B against another build of the library (the profiled child inherits the variable)
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])
torch = None
if not args.launch_only:   # before the first context, as the other probes that share a device with torch do
    try:
        import torch
        if not torch.cuda.is_available():
            torch = None
    except ImportError:
        torch = None
if mp.device_count() < 1:
    raise SystemExit("contours_probe: no HIP device")
CLOCK = "hip events" if torch is not None else "host clock"   # without torch: the host's clock around the synchronous call
n = args.n
nw = n - 2 * mp.OUT_MARGIN
full = (0, 0, 0, 0, 0, 0, nw, nw)
# the rounds, in order: (label, the call on a context, its kernels); every round is reps + contexts calls, the first `contexts` warm up
ROUNDS = [("sim_compare", lambda p: p.sim_compare([full]), ["k_sim", "k_sim_fold"])] + \
         [("sim_contours_%d_%d" % case, lambda p, case=case: p.sim_contours([full], *case), ["k_contour_mask", "k_contour_distance"]) for case in args.cases]
SIZES = {}   # round label -> (contour_a, contour_b) of the last call


def run_rounds(timed):
    """Every round on the rotating contexts; timed(call, p) -> what is kept per call (None: nothing)."""
    ctxs = []
    planes = [phantom(n, seed, noise=4.0) for seed in (1, 2)] if args.content == "phantom" else None
    for k in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        if args.content == "phantom":
            assert p.execute(planes[1]), mp.last_error()
            p.sim_capture(0, 0)
            assert p.execute(planes[0]), mp.last_error()
        else:
            assert p.execute(phantom(n, 1, noise=4.0)), mp.last_error()
            rng = np.random.default_rng(k)
            p.set_image(mp.IMG_GRADED, 0, ((np.pad(rng.integers(0, 256, (nw, nw)), mp.OUT_MARGIN) + 0.5) / 255.0).astype(np.float32))
            p.sim_set_reference(0, rng.integers(0, 256, (nw, nw), dtype=np.uint8) if args.content == "random" else np.full((nw, nw), 77, dtype=np.uint8))
        ctxs.append(p)
    kept = {}
    for label, call, _ in ROUNDS:
        for k in range(args.reps + args.contexts):
            p = ctxs[k % args.contexts]
            v = timed(call, p)
            p.sync()
            if v is not None and k >= args.contexts:
                kept.setdefault(label, []).append(v)
    for p in ctxs:
        p.cleanup()
    return kept


def by_events(call, p):
    if torch is None:
        t0 = time.perf_counter()
        call(p)
        return (time.perf_counter() - t0) * 1e6
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    p.stream_wait(s.cuda_stream)
    call(p)
    p.stream_signal(s.cuda_stream)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def sized(label, call):
    """call, noting the contours' sizes of a sim_contours round."""
    def run(p):
        r = call(p)
        if label.startswith("sim_contours"):
            SIZES[label] = (r[0]["contour_a"], r[0]["contour_b"])
        return r
    return run


ROUNDS = [(label, sized(label, call), kernels) for label, call, kernels in ROUNDS]
if args.launch_only:
    run_rounds(lambda call, p: call(p) and None)
    raise SystemExit(0)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def profiled():
    """{(round label, kernel): [durations in us]} of a --launch-only child under rocprofv3 --kernel-trace; a kernel's launches come in
    its rounds' order, and the first `contexts` launches of each round are dropped."""
    d = tempfile.mkdtemp(prefix="contours_probe_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps), "--contexts", str(args.contexts),
               "--cases", ";".join("%d:%d" % case for case in args.cases), "--content", args.content, "--groups", str(args.groups)]
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("contours_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].replace("void ", "").replace("musica::", "").split("<")[0].split("(")[0]
            times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        per, out, used = args.reps + args.contexts, {}, {}
        for label, _, kernels in ROUNDS:
            for kernel in kernels:
                at = used.get(kernel, 0)
                v = times.get(kernel, [])[at:at + per]
                if len(v) != per:
                    raise SystemExit("contours_probe: %d launches of %s for %s, expected %d" % (len(v), kernel, label, per))
                used[kernel] = at + per
                out[(label, kernel)] = v[args.contexts:]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


if not args.no_launches and shutil.which("rocprofv3") is None:
    raise SystemExit("contours_probe: rocprofv3 not found")
calls = run_rounds(by_events)
launches = None if args.no_launches else profiled()
out = {}
for label, _, kernels in ROUNDS:
    out[label] = {"call_events": summary(calls[label])}
    if label in SIZES:
        out[label]["contours"] = list(SIZES[label])
    if launches is not None:
        out[label]["kernels"] = {k: summary(launches[(label, k)]) for k in kernels}
print(json.dumps({"n": n, "pixels": nw * nw, "content": args.content, "groups": args.groups, "clock": CLOCK, "lib": os.environ.get("PROBE_LIB", ""), "rounds": out}))

"""The cluster metric (kernels_blobs.hip) on the device beside its yardstick, in ONE run on one device.
  call      musica_sim_blobs over the full frame, timed with HIP events around the whole synchronous call (a torch stream that the
            context's stream waits for and signals: musica_stream_wait / musica_stream_signal; where torch finds no device, the
            host's clock around the call, and the output says so), beside musica_sim_compare of the same
            query, which reads the same 4 + 1 bytes a pixel.
  launches  per kernel of the call (k_blobs_tile, k_blobs_seam, k_blobs_flush, k_blobs_flatten with --labels, k_blobs_classify,
            k_blobs_largest) and k_sim / k_sim_fold, from a `rocprofv3 --kernel-trace` run of this script in --launch-only mode (a
            child process).
The scene: the output of image 0 is set to one side and a reference slot to the other side of a random mask of the given densities
(|a - b| in 1 .. 255 on the mask, 0 off it), threshold 0.
Prints one JSON line: per density and connectivity the events' median time of the call and per kernel the calls, the median, the
least and the largest time in us.

The calls rotate over --contexts contexts, one at a time, so that no launch finds its planes in the 256 MiB Infinity Cache.
  python devtools/blobs_probe.py [--n 3072] [--reps 20] [--contexts 6] [--densities 0.0001,0.05,0.40,1.0] [--labels]
  python devtools/blobs_probe.py --launch-only      # what a profiled child runs"""
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
ap.add_argument("--densities", type=lambda s: tuple(float(v) for v in s.split(",")), default=(0.0001, 0.05, 0.40, 1.0))
ap.add_argument("--labels", action="store_true")
ap.add_argument("--launch-only", action="store_true")
args = ap.parse_args()
torch = None
if not args.launch_only:   # before the first context, as the other probes that share a device with torch do
    try:
        import torch
        if not torch.cuda.is_available():
            torch = None
    except ImportError:
        torch = None
if mp.device_count() < 1:
    raise SystemExit("blobs_probe: no HIP device")
CLOCK = "hip events" if torch is not None else "host clock"   # without torch: the host's clock around the synchronous call
n = args.n
nw = n - 2 * mp.OUT_MARGIN
full = (0, 0, 0, 0, 0, 0, nw, nw)
BLOB_KERNELS = ["k_blobs_tile", "k_blobs_seam", "k_blobs_flush"] + (["k_blobs_flatten"] if args.labels else []) + ["k_blobs_classify", "k_blobs_largest"]
# the rounds of a density, in order: (label, the call on a context, its kernels); every round is reps + contexts calls, the first
# `contexts` warm up
ROUNDS = (("sim_compare", lambda p: p.sim_compare([full]), ["k_sim", "k_sim_fold"]),
          ("sim_blobs_4", lambda p: p.sim_blobs([full], 0, 4, labels=args.labels), BLOB_KERNELS),
          ("sim_blobs_8", lambda p: p.sim_blobs([full], 0, 8, labels=args.labels), BLOB_KERNELS))


def sides(density, seed):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((nw, nw)) < density, rng.integers(1, 256, (nw, nw)), 0)
    low = rng.integers(0, 256, d.shape) % (256 - d)
    swap = rng.random(d.shape) < 0.5
    return np.where(swap, low + d, low).astype(np.uint8), np.where(swap, low, low + d).astype(np.uint8)


def run_rounds(timed):
    """Every density's rounds on the rotating contexts; timed(call, p) -> what is kept per call (None: nothing)."""
    ctxs = []
    for _ in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        assert p.execute(phantom(n, 1, noise=4.0)), mp.last_error()
        ctxs.append(p)
    kept = {}
    for density in args.densities:
        for k, p in enumerate(ctxs):
            a, b = sides(density, k)
            p.set_image(mp.IMG_GRADED, 0, ((np.pad(a, mp.OUT_MARGIN) + 0.5) / 255.0).astype(np.float32))
            p.sim_set_reference(0, b)
        for label, call, _ in ROUNDS:
            for k in range(args.reps + args.contexts):
                p = ctxs[k % args.contexts]
                v = timed(call, p)
                p.sync()
                if v is not None and k >= args.contexts:
                    kept.setdefault((density, label), []).append(v)
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


if args.launch_only:
    run_rounds(lambda call, p: call(p) and None)
    raise SystemExit(0)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def profiled():
    """{(density, round label, kernel): [durations in us]} of a --launch-only child under rocprofv3 --kernel-trace; a kernel's launches
    come in its rounds' order, and the first `contexts` launches of each round are dropped."""
    d = tempfile.mkdtemp(prefix="blobs_probe_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps), "--contexts", str(args.contexts),
               "--densities", ",".join(repr(v) for v in args.densities)] + (["--labels"] if args.labels else [])
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("blobs_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].replace("void ", "").replace("musica::", "").split("<")[0].split("(")[0]
            times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        per, out, used = args.reps + args.contexts, {}, {}
        for density in args.densities:
            for label, _, kernels in ROUNDS:
                for kernel in kernels:
                    at = used.get(kernel, 0)
                    v = times.get(kernel, [])[at:at + per]
                    if len(v) != per:
                        raise SystemExit("blobs_probe: %d launches of %s for %s at %g, expected %d" % (len(v), kernel, label, density, per))
                    used[kernel] = at + per
                    out[(density, label, kernel)] = v[args.contexts:]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


if shutil.which("rocprofv3") is None:
    raise SystemExit("blobs_probe: rocprofv3 not found")
calls = run_rounds(by_events)
launches = profiled()
out = {}
for density in args.densities:
    for label, _, kernels in ROUNDS:
        out["%g %s" % (density, label)] = {"call_events": summary(calls[(density, label)]),
                                           "kernels": {k: summary(launches[(density, label, k)]) for k in kernels}}
print(json.dumps({"n": n, "pixels": nw * nw, "labels": args.labels, "clock": CLOCK, "rounds": out}))

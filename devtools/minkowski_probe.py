"""The shape metric (kernels_minkowski.hip) on the device beside its yardstick, in ONE run on one device.
  call      musica_sim_minkowski over the full frame with one query and with four (the frame and three regions one pixel smaller at the
            origins (1, 0), (0, 1), (1, 1)), timed with HIP events around the whole synchronous call (a torch stream that the context's
            stream waits for and signals: musica_stream_wait / musica_stream_signal; where torch finds no device, the host's clock
            around the call, and the output says so), beside musica_sim_compare of the same query, which reads the same 4 + 1 bytes a
            pixel.
  launches  k_minkowski and k_sim / k_sim_fold, from a `rocprofv3 --kernel-trace` run of this script in --launch-only mode (a child
            process); --no-launches leaves that run out.
--contents says what the two sides hold, one set of rounds each:
  random    independent random planes: no two neighbouring cells agree, a run is one cell;
  phantom   the processed output of a phantom on side a and the processed output of another one in the slot;
  constant  both sides 255 everywhere: every cell of a kind wants ONE counter, the contention worst case.
--groups sets MUSICA_MINKOWSKI_GROUPS, the most workgroups of a query's side, for the whole run (0: the launcher's own).
Prints one JSON line and, with --out FILE, writes it there: per content and round the events' median time of the call and per kernel
the calls, the median, the least and the largest time in us.

The calls rotate over --contexts contexts, one at a time, so that no launch finds its planes in the 256 MiB Infinity Cache.
  python devtools/minkowski_probe.py [--n 3072] [--reps 20] [--contexts 6] [--contents random,phantom,constant] [--groups 0] [--no-launches] [--out FILE]
  python devtools/minkowski_probe.py --launch-only      # what a profiled child runs
  PROBE_LIB=<pkg>/libmusica_hip_NAME.so python devtools/minkowski_probe.py ...   # a devtools/build_variant.sh library"""
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

CONTENTS = ("random", "phantom", "constant")
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--contexts", type=int, default=6)
ap.add_argument("--contents", type=lambda s: tuple(s.split(",")), default=CONTENTS)
ap.add_argument("--groups", type=int, default=0)
ap.add_argument("--no-launches", action="store_true")
ap.add_argument("--launch-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if any(c not in CONTENTS for c in args.contents):
    raise SystemExit("minkowski_probe: --contents is a list of %s" % ", ".join(CONTENTS))
if args.groups:
    os.environ["MUSICA_MINKOWSKI_GROUPS"] = str(args.groups)   # read at every call
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
    raise SystemExit("minkowski_probe: no HIP device")
CLOCK = "hip events" if torch is not None else "host clock"   # without torch: the host's clock around the synchronous call
n = args.n
nw = n - 2 * mp.OUT_MARGIN
full = (0, 0, 0, 0, 0, 0, nw, nw)
four = [full] + [(0, 0, x, y, x, y, nw - 1, nw - 1) for x, y in ((1, 0), (0, 1), (1, 1))]
# the rounds, in order: (label, the call on a context, its kernels); every round is reps + contexts calls, the first `contexts` warm up
ROUNDS = [("sim_compare", lambda p: p.sim_compare([full]), ["k_sim", "k_sim_fold"]),
          ("sim_minkowski_1", lambda p: p.sim_minkowski([full]), ["k_minkowski"]),
          ("sim_minkowski_4", lambda p: p.sim_minkowski(four), ["k_minkowski"])]


def run_rounds(content, timed):
    """Every round on the rotating contexts; timed(call, p) -> what is kept per call (None: nothing)."""
    ctxs = []
    planes = [phantom(n, seed, noise=4.0) for seed in (1, 2)] if content == "phantom" else None
    for k in range(args.contexts):
        p = mp.MusicaProcessing()
        assert p.init(n, levels=4, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
        if content == "phantom":
            assert p.execute(planes[1]), mp.last_error()
            p.sim_capture(0, 0)
            assert p.execute(planes[0]), mp.last_error()
        else:
            assert p.execute(phantom(n, 1, noise=4.0)), mp.last_error()
            rng = np.random.default_rng(k)
            a = rng.integers(0, 256, (nw, nw)) if content == "random" else np.full((nw, nw), 255)
            p.set_image(mp.IMG_GRADED, 0, ((np.pad(a, mp.OUT_MARGIN) + 0.5) / 255.0).astype(np.float32))
            p.sim_set_reference(0, rng.integers(0, 256, (nw, nw), dtype=np.uint8) if content == "random" else np.full((nw, nw), 255, dtype=np.uint8))
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


if args.launch_only:
    for content in args.contents:
        run_rounds(content, lambda call, p: call(p) and None)
    raise SystemExit(0)


def summary(v):
    return {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def profiled():
    """{(content, round label, kernel): [durations in us]} of a --launch-only child under rocprofv3 --kernel-trace; a kernel's launches
    come in the contents' and their rounds' order, and the first `contexts` launches of each round are dropped."""
    d = tempfile.mkdtemp(prefix="minkowski_probe_")
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--launch-only", "--n", str(n), "--reps", str(args.reps), "--contexts", str(args.contexts),
               "--contents", ",".join(args.contents), "--groups", str(args.groups)]
        r = subprocess.run([shutil.which("rocprofv3"), "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--"] + cmd,
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("minkowski_probe: the profiled run failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
        rows.sort(key=lambda row: int(row["Start_Timestamp"]))
        times = {}
        for row in rows:
            name = row["Kernel_Name"].replace("void ", "").replace("musica::", "").split("<")[0].split("(")[0]
            times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        per, out, used = args.reps + args.contexts, {}, {}
        for content in args.contents:
            for label, _, kernels in ROUNDS:
                for kernel in kernels:
                    at = used.get(kernel, 0)
                    v = times.get(kernel, [])[at:at + per]
                    if len(v) != per:
                        raise SystemExit("minkowski_probe: %d launches of %s for %s / %s, expected %d" % (len(v), kernel, content, label, per))
                    used[kernel] = at + per
                    out[(content, label, kernel)] = v[args.contexts:]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


if not args.no_launches and shutil.which("rocprofv3") is None:
    raise SystemExit("minkowski_probe: rocprofv3 not found")
calls = {content: run_rounds(content, by_events) for content in args.contents}
launches = None if args.no_launches else profiled()
out = {}
for content in args.contents:
    out[content] = {}
    for label, _, kernels in ROUNDS:
        out[content][label] = {"call_events": summary(calls[content][label])}
        if launches is not None:
            out[content][label]["kernels"] = {k: summary(launches[(content, label, k)]) for k in kernels}
line = json.dumps({"n": n, "pixels": nw * nw, "groups": args.groups, "clock": CLOCK, "lib": os.environ.get("PROBE_LIB", ""), "contents": out})
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)

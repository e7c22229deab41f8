"""Device similarity metrics (musica_sim_compare) against harness.py's numpy ones: one 3052^2 comparison per call, then the whole
metamorphic study (run_study) at 3072^2 / 12 levels with host metrics and with device metrics. Prints one JSON line.
  python devtools/sim_probe.py [--n 3072] [--levels 12] [--calls 200] [--host-reps 2] [--no-study] [--compare-only]
--compare-only: only the device comparisons (for a `rocprofv3 --kernel-trace --stats` run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--levels", type=int, default=12)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--no-study", action="store_true")
ap.add_argument("--compare-only", action="store_true")
args = ap.parse_args()
if mp.device_count() < 1:
    raise SystemExit("sim_probe: no HIP device (the device metrics have no CPU path)")

n = args.n
nw = n - 2 * mp.OUT_MARGIN
out = {"n": n, "levels": args.levels, "pixels": nw * nw, "bytes_per_compare": nw * nw * 5}
raw = phantom(n, 1, noise=4.0)
p = mp.MusicaProcessing()
assert p.init(n, levels=args.levels), mp.last_error()
assert p.execute(raw), mp.last_error()
p.sim_capture(0)
alt = H.add_gaussian_noise(raw, 0.0, 64.0, np.random.default_rng(0))
assert p.execute(alt), mp.last_error()
q = [(0, 0, 0, 0, 0, 0, nw, nw)]
for _ in range(5):
    r = p.sim_compare(q)
t0 = time.perf_counter()
for _ in range(args.calls):
    r = p.sim_compare(q)
out["device_compare_ms"] = (time.perf_counter() - t0) * 1e3 / args.calls   # synchronous call: launches, read-back, host finish
if not args.compare_only:
    a = p.out_pixels(0)                       # the altered output, side a of the timed comparison
    assert p.execute(raw), mp.last_error()
    b = p.out_pixels(0)                       # the unaltered output, what slot 0 holds
    t0 = time.perf_counter()
    for _ in range(args.host_reps):
        host = H.similarities(a, b)
    out["host_compare_ms"] = (time.perf_counter() - t0) * 1e3 / args.host_reps
    out["max_abs_diff_vs_host"] = max(abs(r[0][k] - host[k]) for k in mp.SIM_METRICS)
p.cleanup()

if not (args.no_study or args.compare_only):
    for device in (False, True):
        runner = H.Runner(n, args.levels, device_metrics=device)
        runner.run(raw)                       # warm: code objects, graph capture
        t0 = time.perf_counter()
        rows = H.run_study(raw, runner, rng=np.random.default_rng(0))
        out["study_%s_s" % ("device" if device else "host")] = time.perf_counter() - t0
        out["study_rows"] = len(rows)
        runner.close()
    # the part of a study that is neither metrics nor the pipeline: generating the 31 alterations on the host
    t0 = time.perf_counter()
    rng = np.random.default_rng(0)
    for s in H.scaled(H.SHUTTERS, n):
        H.apply_collimator(raw, s, s, rng)
    for t in H.scaled(H.TRANSLATIONS, n):
        H.clamp_translation(raw, t, 0)
        H.clamp_translation(raw, 0, t)
    for d in H.ROTATIONS:
        H.clamp_rotate(raw, d)
    for sg in H.GAUSS_SIGMAS:
        H.add_gaussian_noise(raw, 0.0, sg, rng)
    for f in H.POISSON_FACTORS:
        H.apply_quantum_noise(raw, f, rng)
    out["alterations_s"] = time.perf_counter() - t0
    out["study_device_over_host"] = out["study_device_s"] / out["study_host_s"]
print(json.dumps(out))

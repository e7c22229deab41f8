"""Device alterations (musica_alter) in the metamorphic study: wall time of one run_study at 3072^2 / 12 levels in three modes (host
metrics, device metrics, device alterations), then per-alteration kernel times from a separate `rocprofv3 --kernel-trace --stats` run of
this script in --alter-only mode (a child process). Prints one JSON line.
  python devtools/alter_probe.py [--n 3072] [--levels 12] [--reps 50] [--skip-host] [--no-profile]
  python devtools/alter_probe.py --alter-only   # only the alterations, each kind --reps times (what the profiled child runs)"""
import argparse
import csv
import glob
import json
import os
import shutil
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

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3072)
ap.add_argument("--levels", type=int, default=12)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--skip-host", action="store_true", help="leave out the host-metrics study (about 26 s at 3072^2)")
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--alter-only", action="store_true")
args = ap.parse_args()
if mp.device_count() < 1:
    raise SystemExit("alter_probe: no HIP device (the device alterations have no CPU path)")

n = args.n
raw = phantom(n, 1, noise=4.0)


def alterations(p):
    """One call per kind, the study's parameters at the largest grid value."""
    return {
        "none": lambda: p.alter_none(),
        "translate_x": lambda: p.alter_translate(H.scaled(H.TRANSLATIONS, n)[-1], 0),
        "translate_y": lambda: p.alter_translate(0, H.scaled(H.TRANSLATIONS, n)[-1]),
        "rotate": lambda: p.alter_rotate(27),
        "collimator": lambda: p.alter_collimator(H.scaled(H.SHUTTERS, n)[0], H.scaled(H.SHUTTERS, n)[0], 1, 1),
        "gaussian": lambda: p.alter_gaussian(0.0, 1024.0, 1, 2),
        "poisson": lambda: p.alter_poisson(0.1, 1, 3),
    }


if args.alter_only:
    p = mp.MusicaProcessing()
    assert p.init(n, levels=args.levels), mp.last_error()
    p.alter_set_source(raw)
    out = {}
    for name, call in alterations(p).items():
        call()
        p.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        p.sync()
        out[name + "_host_ms"] = (time.perf_counter() - t0) * 1e3 / args.reps   # enqueue + kernels, back to back
    p.cleanup()
    print(json.dumps(out))
    raise SystemExit(0)

out = {"n": n, "levels": args.levels, "bytes_per_pass": n * n * 4}
modes = [("device_metrics", dict(device_metrics=True)), ("device_alterations", dict(device_alterations=True))]
if not args.skip_host:
    modes.insert(0, ("host_metrics", {}))
for name, kw in modes:
    runner = H.Runner(n, args.levels, **kw)
    runner.run(raw)                                  # warm: code objects, graph capture
    t0 = time.perf_counter()
    rows = H.run_study(raw, runner, rng=np.random.default_rng(0))
    out["study_%s_s" % name] = time.perf_counter() - t0
    out["study_rows"] = len(rows)
    runner.close()

if not args.no_profile:
    prof = shutil.which("rocprofv3")
    if prof is None:
        out["profile"] = "rocprofv3 not found"
    else:
        d = tempfile.mkdtemp(prefix="alter_probe_")
        cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--alter-only", "--n", str(n), "--levels", str(args.levels), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        out["profile_rc"] = r.returncode
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "k_alter" in name or "k_pct" in name:
                    short = name.split("(")[0].replace("void ", "").replace("musica::", "")
                    kernels[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3}
        out["kernels"] = kernels
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                out["alter_only"] = json.loads(line)
        shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))

"""A few steps of one context as its flags and MUSICA_* knobs make it (lone or MUSICA_FLAG_LINEAR, graph replay where it has it), or of
bench.py's timed form: three contexts of a musica_pipeline in flight. Target of rocprofv3 --kernel-trace; devtools/trace_compare.py
compares the traces of two libraries (PROBE_LIB, as devtools/linear_probe.py).
  python devtools/step_probe.py N L batch [flags]      |      python devtools/step_probe.py pipeline N L batch [flags]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

if os.environ.get("PROBE_LIB"):
    mp.LIB_PATH = os.path.join(ROOT, os.environ["PROBE_LIB"])
pipeline = sys.argv[1] == "pipeline"
args = sys.argv[2:] if pipeline else sys.argv[1:]
n, L, b = (int(a) for a in args[:3])
flags = int(args[3]) if len(args) > 3 else 0
px = np.stack([phantom(n, 100)] * b)   # the launches do not depend on the pixels
steps = int(os.environ.get("PROBE_STEPS", "8"))
if pipeline:
    p = mp.MusicaPipeline(n, levels=L, batch=b, depth=3, flags=flags)
    p.upload(px)
    p.prime()
    for _ in range(3 * steps):
        p.step()
else:
    p = mp.MusicaProcessing()
    assert p.init(n, levels=L, batch=b, flags=flags), mp.last_error()
    p.upload(px)
    for _ in range(steps):
        p.execute_device()
p.sync()
p.cleanup()

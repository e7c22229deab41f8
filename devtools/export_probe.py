"""The device-resident output path (musica_export_out / k_export_u8, tensors.TensorProcessor) against the per-image host path. Prints one
JSON line.
  python devtools/export_probe.py [--iters 200] [--round-trips 30] [--launches-only]

  * export launch: one musica_export_out(MUSICA_OUT_U8) over 8 x 2048^2 and 1 x 3072^2 (back-to-back launches, host clock around a window
    that ends in a device synchronise), against 8 (1) separate k_out_pixels launches (musica_sim_capture launches exactly k_out_pixels for
    one image, with no read-back). The bytes each moves (f32 read of the crop + u8 write) give the share of the 8 TB/s HBM peak;
  * round trip at 8 x 2048^2: torch uint16 on the GPU in, torch uint8 on the GPU out (TensorProcessor: stream_wait, execute_device,
    export_out, stream_signal; one torch.cuda.synchronize at the end of the window) against what a torch caller does without it: the batch
    to the host, musica_execute, musica_get_out_pixels per image and the images back to the GPU.
--launches-only: only the export and k_out_pixels launches (for a `rocprofv3 --kernel-trace --stats` run of their own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libmusica_hip.so then binds to the HIP runtime torch already loaded)

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp  # noqa: E402
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import tensors as T  # noqa: E402
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom_batch  # noqa: E402

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--round-trips", type=int, default=30)
ap.add_argument("--launches-only", action="store_true")
args = ap.parse_args()
if mp.device_count() < 1:
    raise SystemExit("export_probe: no HIP device (the export has no CPU path)")
dev = torch.device("cuda", 0)


def timed(fn, iters, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters


result = {}
for b, n in ((8, 2048), (1, 3072)):
    tp = T.TensorProcessor(n, batch=b, device=dev)
    p = tp.proc
    x = torch.from_numpy(phantom_batch(n, list(range(1, b + 1)))).to(dev)
    torch.cuda.synchronize()
    out = tp(x)
    torch.cuda.synchronize()
    nw = n - 2 * mp.OUT_MARGIN
    moved = b * nw * nw * 5   # 4 B read + 1 B written per output pixel
    ex = timed(lambda: p.export_out(out.data_ptr(), 0, b, mp.OUT_U8), args.iters, p.sync)

    def per_image():
        for k in range(b):
            p.sim_capture(0, k)
    pi = timed(per_image, args.iters, p.sync)
    key = "%dx%d" % (b, n)
    result[key] = {"bytes": moved, "export_u8_us": ex * 1e6, "export_u8_peak_fraction": moved / HBM_PEAK / ex,
                   "out_pixels_launches_us": pi * 1e6, "out_pixels_launches": b, "out_pixels_peak_fraction": moved / HBM_PEAK / pi}
    if not args.launches_only and b == 8:
        rt = timed(lambda: tp(x, out=out), args.round_trips, torch.cuda.synchronize)

        def host_path():
            h = x.cpu().numpy()
            assert p.execute(h)
            imgs = [p.out_pixels(k) for k in range(b)]
            return torch.from_numpy(np.stack(imgs)).to(dev)
        hp = timed(host_path, max(args.round_trips // 3, 3), torch.cuda.synchronize)
        assert torch.equal(tp(x), host_path())
        result[key].update(torch_round_trip_ms=rt * 1e3, torch_round_trip_images_per_s=b / rt,
                           host_path_ms=hp * 1e3, host_path_images_per_s=b / hp)
    tp.cleanup()
print(json.dumps(result))

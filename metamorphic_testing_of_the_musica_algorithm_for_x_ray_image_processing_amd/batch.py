"""Batch driver: independent images sharded one-shard-per-GPU, statistics gathered with one collective.

The reference processes one image per process on one device. A batch of independent images shards
trivially: rank r owns the images `assign_images(total, world)[r]`, runs them through its
own `MusicaProcessing` context with no data-path communication, and at the end one all-gather (RCCL over
xGMI on GPUs, gloo in the CPU tests) collects the fixed-size `musica_stats` row of every image.
Steps in flight on one GPU are the C ABI's musica_pipeline_* (processing.MusicaPipeline).
"""
import ctypes as C

import numpy as np

from .processing import Stats

STATS_WORDS = C.sizeof(Stats) // 4  # 17 x 32-bit words per image


def assign_images(total, world):
    """Image k goes to rank k mod world; returns the list of image ids of every rank."""
    return [list(range(r, total, world)) for r in range(world)]


def stats_to_row(st):
    """One `musica_stats` (ctypes) -> int32[STATS_WORDS] with the struct's exact bytes."""
    return np.frombuffer(bytes(st), dtype=np.int32).copy()


def row_to_stats(row):
    return Stats.from_buffer_copy(np.ascontiguousarray(row, dtype=np.int32).tobytes())


def gather_rows(local_rows, world, dist=None, device=None, force_collective=False):
    """All-gather equal-sized int32 row blocks; returns int32[world * rows, STATS_WORDS] on every rank.

    `local_rows` is a numpy int32 array (CPU / gloo) or a torch tensor already on `device` (GPU / RCCL).
    `force_collective`: run the collective even in a job of one rank (the one-GPU test of the RCCL path).
    """
    import torch
    if isinstance(local_rows, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(local_rows, dtype=np.int32))
        if device is not None:
            t = t.to(device)
    else:
        t = local_rows
    if dist is None or (world == 1 and not force_collective):
        return t                 # one rank: the rows are the job's rows (no copy, no kernel)
    if t.is_cuda and dist.get_backend() == "gloo":
        # one-GPU rehearsal of the multi-rank flow (bench.py --backend gloo): the rows travel through host memory
        parts = [torch.empty(t.shape, dtype=t.dtype) for _ in range(world)]
        dist.all_gather(parts, t.cpu().contiguous())
        return torch.cat(parts).to(t.device)
    out = torch.empty((world * t.shape[0], t.shape[1]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t.contiguous())
    return out


def summarize(rows):
    """Per-image dicts from gathered rows, sorted by image id."""
    out = []
    for r in np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows):
        s = row_to_stats(r)
        out.append({"image_id": int(s.image_id), "min_sqrt": s.min_sqrt, "max_sqrt": s.max_sqrt,
                    "noise_max_bin": [int(v) for v in s.noise_max_bin], "grad_max_bin": int(s.grad_max_bin),
                    "mean_cnr": s.mean_cnr, "t0": s.t0, "ta": s.ta, "t1": s.t1})
    return sorted(out, key=lambda d: d["image_id"])


def process_shard(proc, images, image_ids):
    """Run the images of one rank (batch = proc.batch per execute) and return their stats rows as int32."""
    b = proc.batch
    n = len(image_ids)
    rows = np.zeros((n, STATS_WORDS), dtype=np.int32)
    for start in range(0, n, b):
        chunk = images[start:start + b]
        if len(chunk) < b:  # pad the last chunk by repeating its final image; padded rows are dropped
            chunk = np.concatenate([chunk, np.repeat(chunk[-1:], b - len(chunk), axis=0)])
        if not proc.execute(chunk):
            raise RuntimeError("musica_execute failed")
        for k in range(min(b, n - start)):
            st = proc.stats(k)
            st.image_id = image_ids[start + k]
            rows[start + k] = stats_to_row(st)
    return rows


def process_shard_device(proc, images, image_ids):
    """process_shard on a GPU tensor: `images` is a (n, N, N) torch.uint16 tensor on the context's device (a MusicaProcessing or a
    tensors.TensorProcessor). Returns (rows, outputs) as GPU tensors — int32 (n, STATS_WORDS), the rows process_shard returns, and uint8
    (n, N - 20, N - 20), musica_get_out_pixels' bytes — ordered on the current torch stream, with no host synchronisation and no copy
    to the host. Every chunk goes through one staging batch, so the context replays one captured graph; the last chunk is padded by
    repeating its final image, as process_shard pads it."""
    import torch
    from . import processing as mp
    p = getattr(proc, "proc", proc)
    b, side = p.batch, p.imageSize
    n = len(image_ids)
    if tuple(images.shape) != (n, side, side) or images.dtype != torch.uint16 or images.device.type != "cuda":
        raise ValueError("expected a (%d, %d, %d) torch.uint16 tensor on the GPU, got %r %s on %s" % (n, side, side, tuple(images.shape),
                                                                                                        images.dtype, images.device))
    dev = images.device
    nw = side - 2 * mp.OUT_MARGIN
    chunks = (n + b - 1) // b
    rows = torch.empty((chunks * b, STATS_WORDS), dtype=torch.int32, device=dev)
    outputs = torch.empty((n, nw, nw), dtype=torch.uint8, device=dev)
    stage = torch.empty((b, side, side), dtype=torch.uint16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    src, dst = images.view(torch.int16), stage.view(torch.int16)   # plain copies, whatever kernels torch has for uint16
    for start in range(0, n, b):
        m = min(b, n - start)
        dst[:m].copy_(src[start:start + m])
        if m < b:  # pad the last chunk by repeating its final image; padded rows are dropped
            dst[m:].copy_(src[start + m - 1:start + m].expand(b - m, side, side))
        p.stream_wait(stream)
        try:
            if not p.execute_device(stage.data_ptr()):
                raise RuntimeError("musica_execute_device failed: " + mp.last_error())
            p.export_out(outputs[start].data_ptr(), 0, m, mp.OUT_U8)
            p.stats_device(rows[start].data_ptr())
        finally:
            p.stream_signal(stream)   # the next chunk's copy into `stage` waits for this step
    rows = rows[:n]
    rows[:, 0] = torch.as_tensor(list(image_ids), dtype=torch.int32).to(dev, non_blocking=True)
    return rows, outputs

"""torch tensors in, torch tensors out: the MUSICA path on a uint16 batch that already sits on the GPU, without a host round trip.

    tp = TensorProcessor(2048, batch=8)
    out = tp(x)                     # x: (8, 2048, 2048) torch.uint16 on cuda -> (8, 2028, 2028) torch.uint8 on cuda
    graded = tp(x, output="graded") # -> (8, 2048, 2048) torch.float32 (musica_get_graded's values)

A call is four stream-ordered steps and no host synchronisation: musica_stream_wait(current torch stream), musica_execute_device(x),
musica_export_out(out), musica_stream_signal(same stream). The library's work starts after what the torch stream already holds (the
kernels that produced x), and what torch enqueues on that stream afterwards starts after the library's work. So the caching allocator
cannot hand x or out to another tensor of that stream too early. Using x or out on ANOTHER stream is the caller's job, as for any torch
tensor: `tensor.record_stream(other)` or an explicit event.

The library and torch must run on one HIP runtime (both builds name it libamdhip64.so.7): TensorProcessor imports torch before it loads
libmusica_hip.so, so the library binds to the runtime torch already mapped, and it refuses to start when two are mapped.

Capturing these calls inside torch.cuda.graph is not supported: the library refuses a capturing stream. Graphs of the library's own
step are kept per input pointer (musica_execute_device, four per context): reuse input tensors, or create the processor with
processing.FLAG_NO_GRAPH when more than four input buffers rotate through it.
"""
import ctypes as C
import os

OUTPUTS = ("u8", "graded")


def mapped_hip_runtimes():
    """The distinct files named libamdhip64* mapped into this process (/proc/self/maps)."""
    found = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64"):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


def check_input(x, image_size, batch, device=None):
    """Validates an input batch without touching the library or the GPU: a torch.uint16 tensor of shape (batch, N, N) — or (N, N) when the
    batch is 1 — contiguous, with a 16-byte aligned data_ptr, on a GPU (on `device` when given). Raises TypeError / ValueError."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a torch.Tensor, got %s" % type(x).__name__)
    if x.dtype != torch.uint16:
        raise TypeError("expected a torch.uint16 tensor, got %s" % x.dtype)
    want = (batch, image_size, image_size)
    if tuple(x.shape) != want and not (batch == 1 and tuple(x.shape) == want[1:]):
        raise ValueError("expected shape %r%s, got %r" % (want, " or %r" % (want[1:],) if batch == 1 else "", tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("the input must be contiguous (strided or pitched input is not supported)")
    if x.data_ptr() % 16:
        raise ValueError("the input's data_ptr must be 16-byte aligned (got an address %d bytes past a 16-byte boundary)" % (x.data_ptr() % 16))
    if x.device.type != "cuda":
        raise ValueError("the input must be on the GPU, got a tensor on %s" % x.device)
    if device is not None and x.device != torch.device(device):
        raise ValueError("the input is on %s, the processor runs on %s" % (x.device, torch.device(device)))


def check_output(out, shape, dtype, device=None):
    """Validates a caller's output tensor (rows may be strided: stride(-1) == 1, stride(-2) >= the row's width, images apart by at least
    a whole image) and returns its (row pitch, image pitch) in bytes. Raises TypeError / ValueError."""
    import torch
    if not isinstance(out, torch.Tensor):
        raise TypeError("out: expected a torch.Tensor, got %s" % type(out).__name__)
    if out.dtype != dtype:
        raise TypeError("out: expected %s, got %s" % (dtype, out.dtype))
    if tuple(out.shape) != tuple(shape):
        raise ValueError("out: expected shape %r, got %r" % (tuple(shape), tuple(out.shape)))
    rows, width = shape[-2], shape[-1]
    if out.stride(-1) != 1 or out.stride(-2) < width:
        raise ValueError("out: rows must be dense with a row stride of at least %d elements, got strides %r" % (width, out.stride()))
    image_stride = out.stride(0) if out.dim() == 3 else out.stride(-2) * rows
    if out.dim() == 3 and shape[0] > 1 and image_stride < out.stride(-2) * rows:
        raise ValueError("out: images overlap (image stride %d < %d rows x %d)" % (image_stride, rows, out.stride(-2)))
    if out.device.type != "cuda":
        raise ValueError("out must be on the GPU, got a tensor on %s" % out.device)
    if device is not None and out.device != torch.device(device):
        raise ValueError("out is on %s, the processor runs on %s" % (out.device, torch.device(device)))
    item = out.element_size()
    return out.stride(-2) * item, max(image_stride, out.stride(-2) * rows) * item


class TensorProcessor:
    """One MUSICA context fed from and writing to torch tensors on one GPU (see the module docstring for the ordering guarantees)."""

    def __init__(self, image_size, levels=0, batch=1, flags=0, device=None, tunables=None):
        import torch            # first: libmusica_hip.so then binds to the HIP runtime torch already loaded
        from . import processing as mp
        self._mp = mp
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device.index if isinstance(device, torch.device) else int(device))
        mp.load_library()
        runtimes = mapped_hip_runtimes()
        if len(runtimes) > 1:
            raise RuntimeError("more than one HIP runtime is mapped into this process (%s): torch and libmusica_hip.so must share one"
                               % ", ".join(runtimes))
        self.proc = mp.MusicaProcessing(device=self.device.index)
        if not self.proc.init(int(image_size), levels=levels, batch=batch, flags=flags, tunables=tunables):
            raise RuntimeError("musica_create failed: " + mp.last_error())
        self.image_size = self.proc.imageSize
        self.batch = self.proc.batch
        self.stats_words = C.sizeof(mp.Stats) // 4

    def out_shape(self, output="u8", single=False):
        n = self.image_size
        side = n - 2 * self._mp.OUT_MARGIN if output == "u8" else n
        return (side, side) if single else (self.batch, side, side)

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def __call__(self, x, out=None, output="u8"):
        """x: (batch, N, N) torch.uint16 on the processor's GPU ((N, N) when the batch is 1). Returns `out` (allocated when None):
        (batch, N - 20, N - 20) torch.uint8 for output="u8" — musica_get_out_pixels' bytes — or (batch, N, N) torch.float32 for
        output="graded"; two-dimensional when x is. Ordered on the current torch stream; nothing waits on the host."""
        import torch
        if output not in OUTPUTS:
            raise ValueError("output must be one of %r, got %r" % (OUTPUTS, output))
        check_input(x, self.image_size, self.batch, self.device)
        fmt, dtype = (self._mp.OUT_U8, torch.uint8) if output == "u8" else (self._mp.OUT_GRADED_F32, torch.float32)
        shape = self.out_shape(output, single=x.dim() == 2)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        row_pitch, image_pitch = check_output(out, shape, dtype, self.device)
        stream = self._stream()
        self.proc.stream_wait(stream)
        try:
            if not self.proc.execute_device(x.data_ptr()):
                raise RuntimeError("musica_execute_device failed: " + self._mp.last_error())
            self.proc.export_out(out.data_ptr(), 0, self.batch, fmt, row_pitch, image_pitch)
        finally:
            self.proc.stream_signal(stream)   # whatever was enqueued, the torch stream waits for it before x / out may be reused
        return out

    def stats(self, out=None, image_id_base=0, image_id_stride=1):
        """The musica_stats rows of the last call as a (batch, stats_words) torch.int32 tensor on the GPU (musica_stats_device), ordered on
        the current torch stream like __call__; image_id = image_id_base + index * image_id_stride."""
        import torch
        shape = (self.batch, self.stats_words)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError("out: expected a contiguous %r torch.int32 tensor on %s" % (shape, self.device))
        stream = self._stream()
        self.proc.stream_wait(stream)
        try:
            self.proc.stats_device(out.data_ptr(), image_id_base, image_id_stride)
        finally:
            self.proc.stream_signal(stream)
        return out

    def cleanup(self):
        """Destroys the context (it waits for its own stream first)."""
        self.proc.cleanup()

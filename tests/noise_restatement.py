"""A host restatement of the noise draws of the device alterations (test infrastructure, next to golden_util.py).

Written from the contract, not from the kernel: include/musica.h ("alterations of the metamorphic study"), DESIGN.md section 4
("Alterations of the study on the device"), Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC 2011) for Philox4x32-10
and W. Hormann, "The transformed rejection method for generating Poisson random variables" (1993) for PTRS. Everything is numpy on
arrays of pixels; the samplers loop over rounds with the set of pixels that are still drawing.

The contract in short:
  * key = (seed & 0xffffffff, seed >> 32); block j (j = 0, 1, ..) of pixel p (its row-major index in the N x N plane) is
    Philox4x32-10 of the counter (p, j, stream, 0) under that key, with output words (x, y, z, w);
  * a block yields two uniforms in [0, 1): u53(x, y) first, then u53(z, w), where u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) / 2^53;
    so uniform number t of a pixel is half t & 1 of block t >> 1, and a pixel's draws depend on (seed, stream, p) and the values
    the sampler sees, never on the image side, the batch index or the launch;
  * normal: Box-Muller in f64 on the pixel's uniforms number 0 and 1, z = sqrt(-2 ln(1 - u_0)) cos(2 pi u_1), the draw is
    mean + sigma z truncated toward zero and saturated to int32;
  * Poisson(lam): 0 when lam is not > 0; below 10 the number of uniforms multiplied together before the product is no longer
    above exp(-lam), minus one (Knuth; one uniform per round); from 10 on Hormann's PTRS (two uniforms per round: U = u - 0.5 first,
    then V).

FRAGILE PIXELS. The device evaluates exp, log, cos and lgamma with its own libm (and may contract a * b + c into one fma), so a
draw can legitimately differ from this file's where a comparison or a floor / trunc sits within a few ulp of its threshold. Each
sampler therefore also returns a mask of such pixels: those where the truncated normal value lies within FRAGILE_WINDOW, relative
to the magnitudes that were added, of a non-zero integer (truncation toward zero does not change at 0), or where a Poisson
accept / reject comparison or PTRS's floor argument lies within that window of its threshold. The device libm's error on gfx950
has not been measured here; FRAGILE_WINDOW = 2^-36 is some 2^16 ulp of f64, far above any documented error of a device function
(a few ulp), and still small enough that a 513 x 513 plane holds a handful of fragile pixels at most. A caller compares every other
pixel exactly and bounds the number of fragile ones (MAX_FRAGILE per plane): a condition on the inputs, not on the kernel."""
import numpy as np
from scipy import special

FRAGILE_WINDOW = 2.0 ** -36
MAX_FRAGILE = 16

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)     # the two multipliers of Philox4x32
_W0, _W1 = 0x9E3779B9, 0xBB67AE85                           # the key schedule's Weyl increments (golden ratio, sqrt(3) - 1)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds. counter: (..., 4) and key: (..., 2) (broadcast against each other) of 32-bit words; returns the
    (..., 4) uint32 output words."""
    c = np.asarray(counter).astype(np.uint64) & _LOW
    k = np.asarray(key).astype(np.uint64) & _LOW
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LOW, (p0 >> _S32) ^ c3 ^ k1, p0 & _LOW
        k0, k1 = (k0 + np.uint64(_W0)) & _LOW, (k1 + np.uint64(_W1)) & _LOW
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def u53(a, b):
    """A uniform double in [0, 1) from two 32-bit words: the top 27 bits of a, then the top 26 bits of b."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


class PixelStreams:
    """The uniform streams of an array of pixels: uniform number t of pixel p is half t & 1 of block t >> 1 = Philox(counter
    (p, t >> 1, stream, 0), key (seed low word, seed high word))."""

    def __init__(self, pixels, seed, stream):
        self.pixels = np.asarray(pixels, dtype=np.uint64).ravel()
        self.key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
        self.stream = int(stream) & 0xFFFFFFFF
        self.used = np.zeros(self.pixels.size, dtype=np.int64)   # uniforms consumed so far, per pixel

    def next(self, idx):
        """The next uniform of each pixel in `idx` (indices into the array given to the constructor)."""
        t = self.used[idx]
        ctr = np.zeros((len(idx), 4), dtype=np.uint64)
        ctr[:, 0] = self.pixels[idx]
        ctr[:, 1] = t >> 1
        ctr[:, 2] = self.stream
        out = philox4x32_10(ctr, self.key)
        second = (t & 1) == 1
        self.used[idx] = t + 1
        return np.where(second, u53(out[:, 2], out[:, 3]), u53(out[:, 0], out[:, 1]))


def _near(x, threshold, scale):
    return np.abs(x - threshold) <= FRAGILE_WINDOW * scale


def gauss_draw(mean, sigma, pixels, seed, stream):
    """(draws int32, fragile bool), one per pixel: trunc(mean + sigma z) saturated to int32, z by Box-Muller on 1 - u_0 and u_1."""
    g = PixelStreams(pixels, seed, stream)
    every = np.arange(g.pixels.size)
    u1 = 1.0 - g.next(every)                                 # (0, 1]: the logarithm is finite
    u2 = g.next(every)
    radius = np.sqrt(-2.0 * np.log(u1))
    x = mean + sigma * (radius * np.cos(2.0 * np.pi * u2))
    nearest = np.rint(x)
    fragile = (nearest != 0.0) & _near(x, nearest, abs(mean) + abs(sigma) * radius)
    draws = np.clip(np.trunc(x), -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32)
    return draws, fragile


def poisson_draw(lam, pixels, seed, stream):
    """(draws int64, fragile bool), one per pixel, for the per-pixel means `lam` (f64)."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    g = PixelStreams(pixels, seed, stream)
    assert lam.size == g.pixels.size
    draws = np.zeros(lam.size, dtype=np.int64)               # lam not > 0 (NaN included): 0, and no uniform is consumed
    fragile = np.zeros(lam.size, dtype=bool)
    positive = lam > 0.0

    # below 10: multiply uniforms until the product is no longer above exp(-lam)
    idx = np.flatnonzero(positive & (lam < 10.0))
    floor_p = np.exp(-lam[idx])
    prod = np.ones(idx.size)
    rounds = 0
    while idx.size:
        prod = prod * g.next(idx)
        fragile[idx] |= _near(prod, floor_p, np.maximum(prod, floor_p))
        go_on = prod > floor_p
        draws[idx[~go_on]] = rounds
        idx, prod, floor_p = idx[go_on], prod[go_on], floor_p[go_on]
        rounds += 1
        assert rounds < 4096, "the inversion below lambda = 10 does not end"

    # from 10 on: PTRS (Hormann 1993, algorithm PTRS; the constants are the paper's)
    idx = np.flatnonzero(positive & (lam >= 10.0))
    rounds = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while idx.size:
            m = lam[idx]
            slam, loglam = np.sqrt(m), np.log(m)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            U = g.next(idx) - 0.5
            V = g.next(idx)
            us = 0.5 - np.abs(U)
            step = (2.0 * a / us + b) * U
            arg = step + m + 0.43
            k = np.floor(arg)
            finite = np.isfinite(arg)
            frag = finite & (_near(arg, k, np.abs(step) + m + 0.43) | _near(arg, k + 1.0, np.abs(step) + m + 0.43))
            central = us >= 0.07                             # exact on both sides: us is 0.5 - |u - 0.5|
            frag |= central & _near(V, vr, 1.0)
            quick = central & (V <= vr)
            again = ~quick & ((k < 0.0) | ((us < 0.013) & (V > us)))   # V > us compares two exact numbers
            test = ~quick & ~again
            kt = np.where(test, k, 0.0)
            t_v, t_alpha, t_h = np.log(V), np.log(inv_alpha), np.log(a / (us * us) + b)
            t_k, t_g = kt * loglam, special.gammaln(kt + 1.0)
            lhs = t_v + t_alpha - t_h
            rhs = -m + t_k - t_g
            scale = np.abs(t_v) + np.abs(t_alpha) + np.abs(t_h) + m + np.abs(t_k) + np.abs(t_g)
            frag |= test & _near(lhs, rhs, scale)
            accept = quick | (test & (lhs <= rhs))
            fragile[idx] |= frag
            draws[idx[accept]] = k[accept].astype(np.int64)
            idx = idx[~accept]
            rounds += 1
            assert rounds < 4096, "PTRS does not end"
    return draws, fragile


# ---- the three alterations that draw (harness.add_gaussian_noise, apply_quantum_noise, apply_collimator) ---------------------------

def restate_gaussian(src, mean, sigma, seed, stream):
    """(draws (N, N) int32, altered (N, N) uint16, fragile (N, N) bool): clip(v + draw, 0, 65535)."""
    src = np.asarray(src, dtype=np.uint16)
    e, fragile = gauss_draw(float(mean), float(sigma), np.arange(src.size), seed, stream)
    out = np.clip(src.astype(np.int64).ravel() + e, 0, 65535).astype(np.uint16)
    return e.reshape(src.shape), out.reshape(src.shape), fragile.reshape(src.shape)


def restate_poisson(src, factor, seed, stream):
    """(draws k ~ Poisson(v * factor) as int32, altered, fragile): float32(k) / float32(factor), clipped to [0, 65535], truncated."""
    src = np.asarray(src, dtype=np.uint16)
    k, fragile = poisson_draw(src.astype(np.float64).ravel() * float(factor), np.arange(src.size), seed, stream)
    out = np.clip(k.astype(np.float32) / np.float32(factor), 0, 65535).astype(np.uint16)
    return k.astype(np.int32).reshape(src.shape), out.reshape(src.shape), fragile.reshape(src.shape)


def collimator_inside(n, shutter_h, shutter_v):
    """The inclusive rectangle apply_collimator keeps: rows shutter_v .. N - shutter_v, columns shutter_h .. N - shutter_h."""
    inside = np.zeros((n, n), dtype=bool)
    inside[shutter_v:n - shutter_v + 1, shutter_h:n - shutter_h + 1] = True
    return inside


def restate_collimator(src, shutter_h, shutter_v, seed, stream):
    """(draws k ~ Poisson(v / 100) of EVERY pixel as int32, altered, fragile): the source inside the rectangle, min(k, 65535) outside.
    `fragile` is the draws'; the altered image can differ from this one only where fragile & ~inside."""
    src = np.asarray(src, dtype=np.uint16)
    k, fragile = poisson_draw(src.astype(np.float64).ravel() / 100.0, np.arange(src.size), seed, stream)
    inside = collimator_inside(src.shape[0], shutter_h, shutter_v)
    out = np.where(inside, src, np.minimum(k, 65535).astype(np.uint16).reshape(src.shape))
    return k.astype(np.int32).reshape(src.shape), out, fragile.reshape(src.shape)


# ---- the planes the GPU test draws (tests/test_gpu_noise_draws.py); tests/test_noise_restatement.py bounds their fragile counts ------

def draw_source(n):
    """An N x N source with rows of 0 (lambda = 0), rows of 65535, a band of small values (lambda on both sides of 10 for the
    factors below, lambda < 10 under the collimator's v / 100) and the full range elsewhere."""
    rng = np.random.default_rng(1000 + n)
    src = rng.integers(0, 65536, (n, n), dtype=np.uint16)
    src[:8] = 0
    src[8:16] = 65535
    src[16:n // 2] = rng.integers(0, 300, (n // 2 - 16, n), dtype=np.uint16)
    return src


HI = 0x9E3779B9 << 32          # a non-zero high word for the seeds

# (side, image_index, kind, arguments, seed, stream). The odd side's planes are stored by k_alter's scalar branch.
DRAW_CASES = (
    [(513, k & 1, "gaussian", dict(mean=m, sigma=s), HI | 12, 2) for k, (s, m) in enumerate(((4.0, 0.0), (1024.0, 0.0), (30000.0, 0.0), (16.0, -3.5)))] +
    [(513, 0, "gaussian", dict(mean=0.0, sigma=256.0), (1 << 32) | 7, 4),       # two seeds that differ in the high word only
     (513, 1, "gaussian", dict(mean=0.0, sigma=256.0), (2 << 32) | 7, 4),
     (513, 1, "gaussian", dict(mean=0.0, sigma=256.0), (2 << 32) | 7, 5)] +      # ... and two streams
    [(513, k & 1, "poisson", dict(factor=f), HI | 11, 1) for k, f in enumerate((0.1, 0.3, 0.7, 0.00625, 3.0, 1.0 / 3.0, 0.05))] +
    [(513, 1, "poisson", dict(factor=0.1), (1 << 32) | 11, 1),
     (513, 0, "poisson", dict(factor=0.1), HI | 11, 6),
     (513, 0, "collimator", dict(shutter_h=40, shutter_v=43), HI | 13, 3),
     (513, 1, "collimator", dict(shutter_h=60, shutter_v=60), 13, 4),
     (513, 1, "collimator", dict(shutter_h=0, shutter_v=256), 13, 4),          # the widest outside an odd side allows
     (512, 0, "gaussian", dict(mean=0.0, sigma=64.0), HI | 5, 2),
     (512, 1, "poisson", dict(factor=0.1), HI | 11, 1),
     (512, 1, "collimator", dict(shutter_h=40, shutter_v=43), HI | 13, 3)]
)


def restate_case(src, kind, args, seed, stream):
    fn = {"gaussian": restate_gaussian, "poisson": restate_poisson, "collimator": restate_collimator}[kind]
    return fn(src, seed=seed, stream=stream, **args)

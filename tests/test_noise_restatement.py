"""CPU checks of the host restatement of the noise draws (tests/noise_restatement.py): Philox4x32-10 against Random123's known-answer
vectors, the uniform stream's layout, the samplers' distributions (so the restatement itself is a Poisson / normal sampler and not
merely something the device agrees with), and the fragile count of every plane tests/test_gpu_noise_draws.py draws. No GPU needed."""
import numpy as np
import pytest
from scipy import special

import noise_restatement as NR

# Random123 kat_vectors, "philox4x32 10": counter, key, output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = NR.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # on arrays: the three vectors at once, each under its own key
    got = NR.philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint64), np.array([k[1] for k in KAT], dtype=np.uint64))
    assert got.dtype == np.uint32 and np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))


def test_u53_uses_27_and_26_bits():
    assert NR.u53(0, 0) == 0.0
    assert NR.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert NR.u53(1 << 5, 0) == 2.0 ** -27 and NR.u53(31, 63) == 0.0      # the low 5 and 6 bits are dropped
    assert NR.u53(0, 1 << 6) == 2.0 ** -53 and NR.u53(0x80000000, 0) == 0.5


def test_pixel_stream_layout():
    """Uniform t of pixel p is half t & 1 of the block with counter (p, t >> 1, stream, 0) under key (seed low, seed high)."""
    seed, stream = (0xA4093822 << 32) | 0x299F31D0, 7
    pixels = np.array([0, 5, 70000], dtype=np.uint64)
    g = NR.PixelStreams(pixels, seed, stream)
    drawn = np.stack([g.next(np.arange(3)) for _ in range(4)])            # uniforms 0 .. 3 of the three pixels
    for col, p in enumerate(pixels):
        for j in range(2):
            x, y, z, w = NR.philox4x32_10(np.array([int(p), j, stream, 0], dtype=np.uint64), np.array([0x299F31D0, 0xA4093822], dtype=np.uint64))
            assert drawn[2 * j, col] == NR.u53(x, y) and drawn[2 * j + 1, col] == NR.u53(z, w)
    # pixels advance independently
    g = NR.PixelStreams(pixels, seed, stream)
    a = g.next(np.array([1]))
    b = g.next(np.array([0, 1]))
    assert a[0] == drawn[0, 1] and b[0] == drawn[0, 0] and b[1] == drawn[1, 1]


def _trunc_normal_moments(mean, sigma):
    """E, Var and the 4th central moment of trunc(N(mean, sigma)), by summing its pmf: trunc(x) == k for x in [k, k + 1) when k > 0,
    (k - 1, k] when k < 0, (-1, 1) when k == 0."""
    k = np.arange(int(mean - 12 * sigma) - 2, int(mean + 12 * sigma) + 3)
    lo = np.where(k > 0, k, np.where(k < 0, k - 1, -1)).astype(np.float64)
    hi = np.where(k > 0, k + 1, np.where(k < 0, k, 1)).astype(np.float64)
    pmf = special.ndtr((hi - mean) / sigma) - special.ndtr((lo - mean) / sigma)
    m = np.sum(pmf * k)
    var = np.sum(pmf * (k - m) ** 2)
    return m, var, np.sum(pmf * (k - m) ** 4)


def test_samplers_follow_their_distributions():
    size = 1 << 17
    px = np.arange(size)
    for lam in (0.3, 4.0, 9.9, 10.0, 10.1, 37.0, 655.0, 6553.5):
        k, fragile = NR.poisson_draw(np.full(size, lam), px, 77, int(lam * 10))
        assert fragile.sum() <= NR.MAX_FRAGILE
        assert abs(k.mean() - lam) < 5 * np.sqrt(lam / size), (lam, k.mean())
        assert abs(k.var() - lam) < 5 * np.sqrt((lam + 2 * lam * lam) / size), (lam, k.var())
    k, fragile = NR.poisson_draw(np.array([0.0, -1.0, np.nan]), np.arange(3), 1, 1)
    assert not k.any() and not fragile.any()
    for mean, sigma in ((0.0, 1024.0), (-3.5, 16.0)):
        e, fragile = NR.gauss_draw(mean, sigma, px, 78, 1)
        assert fragile.sum() <= NR.MAX_FRAGILE
        m, var, m4 = _trunc_normal_moments(mean, sigma)
        assert abs(e.mean() - m) < 5 * np.sqrt(var / size), (sigma, e.mean(), m)
        assert abs(e.var() - var) < 5 * np.sqrt((m4 - var * var) / size), (sigma, e.var(), var)
    e, _ = NR.gauss_draw(0.0, 1e12, px, 78, 1)                              # saturates at both ends of int32
    assert e.min() == -2 ** 31 and e.max() == 2 ** 31 - 1


def test_keys_and_streams_separate_the_draws():
    px = np.arange(4096)
    base, _ = NR.gauss_draw(0.0, 256.0, px, (1 << 32) | 7, 4)
    for seed, stream in (((2 << 32) | 7, 4), ((1 << 32) | 8, 4), ((1 << 32) | 7, 5)):
        other, _ = NR.gauss_draw(0.0, 256.0, px, seed, stream)
        assert (other != base).mean() > 0.9, (seed, stream)
    again, _ = NR.gauss_draw(0.0, 256.0, px[::-1], (1 << 32) | 7, 4)       # a pixel's draw follows its index, not its position
    assert np.array_equal(again[::-1], base)


@pytest.mark.parametrize("case", range(len(NR.DRAW_CASES)))
def test_fragile_count_of_every_gpu_plane(case):
    """The planes of tests/test_gpu_noise_draws.py hold at most MAX_FRAGILE pixels whose draw the device may round the other way."""
    n, _, kind, args, seed, stream = NR.DRAW_CASES[case]
    draws, out, fragile = NR.restate_case(NR.draw_source(n), kind, args, seed, stream)
    print("case %d %s %r: %d fragile of %d" % (case, kind, args, int(fragile.sum()), fragile.size))
    assert draws.shape == out.shape == fragile.shape == (n, n)
    assert fragile.sum() <= NR.MAX_FRAGILE, (kind, args, int(fragile.sum()))

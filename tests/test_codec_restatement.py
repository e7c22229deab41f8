"""The exact 8 x 8 block codec as the metrics state it (block_codec, codec_table, codec_table8), the constants and prototypes that carry
it to the library, the host path of a study with `codecs` and the --codecs argument: everything that needs no GPU.

block_codec is the contract of musica_alter_codec and musica_sim_codec_reference (include/musica.h); here it is held to a literal second
restatement in nested loops and Python ints (codec_restatement.py), and its int32 bounds are asserted where they are tightest.

Nothing here asserts how much of a codec's loss the pipeline passes on or amplifies: the similarities of a codec_* row are findings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import metrics
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

import codec_restatement as R
from codec_restatement import StubRunner

ONES = np.ones((8, 8), np.int64)
TWOS = np.full((8, 8), 2, np.int64)
TOP = np.full((8, 8), 65535, np.int64)
PRIMES = np.array([3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131, 137,
                   139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199, 211, 223, 227, 229, 233, 239, 241, 251, 257, 263, 269, 271, 277, 281,
                   283, 293, 307, 311, 313]).reshape(8, 8)   # 64 distinct odd primes: no two coefficients share a step


def _noise(n, dtype, seed):
    top = np.iinfo(dtype).max
    a = np.random.default_rng(seed).integers(0, top + 1, (n, n), dtype=dtype)
    a.flat[0], a.flat[-1] = 0, top
    return a


def _loops(plane, table, origin=(0, 0), seen=None):
    out = R.block_codec(plane.tolist(), np.asarray(table).tolist(), origin, 8 * plane.dtype.itemsize, seen)
    return np.array(out, dtype=plane.dtype)


def test_the_matrix_is_the_rounded_cosines_typed_twice():
    assert H.CODEC_M.tolist() == R.M == R.matrix_from_the_cosines()
    assert H.CODEC_M.dtype == np.int64 and int(np.abs(H.CODEC_M).sum(axis=0).max()) == 3825
    assert (H.CODEC_M[1:].sum(axis=1) == 0).all()          # a constant row has no AC part, exactly
    assert metrics.block_codec is H.block_codec and metrics.codec_table is H.codec_table   # harness re-exports the contract


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("n, origin", [(8, (0, 0)), (16, (0, 0)), (9, (0, 0)), (13, (2, 2)), (20, (7, 0)), (11, (0, 7)), (3, (5, 6)), (1, (0, 0))])
def test_block_codec_is_the_nested_loops(n, origin, dtype):
    x = _noise(n, dtype, 10 * n + origin[0])
    for table in (ONES, TWOS, PRIMES, H.codec_table(256), TOP):
        got = H.block_codec(x, table, origin)
        assert got.dtype == x.dtype and got.shape == x.shape
        assert np.array_equal(got, _loops(x, table, origin)), (n, origin, int(np.asarray(table)[0, 0]))


def _sign_planes():
    """The 64 planes where(sign(outer(M[u], M[v])) > 0, 65535, 0): every pixel pushes coefficient (u, v) the same way."""
    M = H.CODEC_M
    return np.stack([np.where(np.sign(np.outer(M[u], M[v])) > 0, 65535, 0) for u in range(8) for v in range(8)]).astype(np.int64)


def test_the_int32_bounds_on_the_sign_planes():
    X = _sign_planes() - 32768
    for table in (ONES, TOP, PRIMES):
        s = H.codec_blocks(X, np.asarray(table, np.int64))
        assert np.abs(s["XMt"]).max() <= 1 << 27
        assert np.abs(s["MA"]).max() <= 1 << 29
        assert np.abs(s["F"]).max() <= 1 << 18
        assert np.abs(s["Fq"]).max() <= (1 << 18) + 32767
        assert np.abs(s["MtF"]).max() < 1 << 31
        assert np.abs(s["A2M"]).max() <= 1 << 30
        assert np.abs(s["A2"]).max() <= 1 << 18
    # the same stages, seen by the loops
    seen = {}
    for plane in _sign_planes():
        R.codec_block((plane - 32768).tolist(), ONES.tolist(), seen)
    assert seen["XMt"] <= 1 << 27 and seen["MA"] <= 1 << 29 and seen["F"] <= 1 << 18 and seen["MtF"] < 1 << 31 and seen["A2M"] <= 1 << 30
    assert seen["MA"] == int(np.abs(H.codec_blocks(X, ONES)["MA"]).max())


def test_the_int32_bound_on_the_adversarial_coefficients():
    """F' at its largest magnitude with the signs of one column of M: |M^T F'| = 3825 (2^18 + 32767) < 2^31, and the clamp catches it."""
    M, big = H.CODEC_M, (1 << 18) + 32767
    worst = 0
    for y in range(8):
        Fq = np.sign(M[:, y])[:, None] * np.full((8, 8), big, np.int64)
        raw = M.T @ Fq
        worst = max(worst, int(np.abs(raw).max()))
        a2 = np.clip((raw + 512) >> 10, -(1 << 18), (1 << 18) - 1)
        assert a2.max() == (1 << 18) - 1 and int(np.abs(a2 @ M).max()) <= 1 << 30
        py = sum(int(M[v, y]) * int(Fq[v, 0]) for v in range(8))
        assert py == int(raw[y, 0])
    assert worst == 3825 * big == 1128034575 and worst < 1 << 31
    assert int(np.abs(M).sum(axis=1).max()) * (1 << 18) <= 1 << 30     # |A' M| with A' at the clamp


@pytest.mark.parametrize("v, steps", [(0, (1, 2, 256, 4096, 32768)), (12345, (1, 2, 4, 8, 13, 1571)), (65535, (1, 2, 4, 8, 7, 31, 56, 151))])
def test_a_constant_plane_comes_back_when_the_dc_step_divides(v, steps):
    X = v - 32768
    rng = np.random.default_rng(v)
    for n, origin in ((44, (0, 0)), (16, (0, 0)), (13, (3, 5))):
        flat = np.full((n, n), v, np.uint16)
        for s in steps:
            assert (8 * X) % s == 0
            table = rng.integers(1, 65536, (8, 8))
            table[0, 0] = s
            assert np.array_equal(H.block_codec(flat, table, origin), flat), (v, s, n)
    if v == 0:   # a collimated zero region stays zero under every table of the study
        for s in H.CODECS:
            assert np.array_equal(H.block_codec(np.zeros((24, 24), np.uint16), H.codec_table(s)), np.zeros((24, 24), np.uint16))


def test_halves_round_away_from_zero_for_both_signs():
    x = _noise(40, np.uint16, 3)
    assert np.array_equal(H.block_codec(x, TWOS), _loops(x, TWOS))
    blocks = x.astype(np.int64).reshape(5, 8, 5, 8).transpose(0, 2, 1, 3) - 32768
    s = H.codec_blocks(blocks, TWOS)
    odd = s["F"] % 2 != 0
    assert 0.4 < odd.mean() < 0.6                                  # half the coefficients sit on a rounding half
    assert (s["F"][odd] > 0).any() and (s["F"][odd] < 0).any()
    assert np.array_equal(np.abs(s["Fq"][odd]), np.abs(s["F"][odd]) + 1)
    assert np.array_equal(s["Fq"][~odd], s["F"][~odd])


def test_the_origin_moves_the_blocks():
    x = _noise(40, np.uint16, 4)
    t = H.codec_table(1024)
    assert not np.array_equal(H.block_codec(x, t, (2, 2)), H.block_codec(x, t))
    # the plane at origin (2, 2) is the interior of a plane that starts two pixels earlier on the same grid
    big = np.pad(x, ((2, 6), (2, 6)), mode="edge")
    assert np.array_equal(H.block_codec(x, t, (2, 2)), H.block_codec(big, t)[2:42, 2:42])
    x8 = _noise(24, np.uint8, 5)
    t8 = H.codec_table8(t)
    assert not np.array_equal(H.block_codec(x8, t8, (2, 2)), H.block_codec(x8, t8))


@pytest.mark.parametrize("n", [44, 137])
def test_a_block_that_sticks_out_is_completed_by_edge_replication(n):
    x = _noise(n, np.uint16, n)
    t = H.codec_table(256)
    got = H.block_codec(x, t)
    assert np.array_equal(got, _loops(x, t))
    m = -(-n // 8) * 8
    assert np.array_equal(got, H.block_codec(np.pad(x, ((0, m - n), (0, m - n)), mode="edge"), t)[:n, :n])
    x8 = _noise(n, np.uint8, n + 1)
    assert np.array_equal(H.block_codec(x8, H.codec_table8(t), (2, 2)), _loops(x8, H.codec_table8(t), (2, 2)))


def test_the_study_tables():
    K = H.CODEC_K
    assert K.shape == (8, 8) and K[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and K[7].tolist() == [72, 92, 95, 98, 112, 100, 103, 99]
    assert H.CODECS == (16, 64, 256, 1024, 4096)
    for s in H.CODECS + (1, 3, 65535):
        t = H.codec_table(s)
        assert t.dtype == np.uint16 and t.shape == (8, 8) and int(t[0, 0]) == s
        assert np.array_equal(t, np.clip((K * s + 8) >> 4, 1, 65535))
    assert np.array_equal(H.codec_table(16), K)                       # the table itself
    assert np.array_equal(H.codec_table8(H.codec_table(4096)), K)     # the 8-bit quality-50 table at 16-bit scale, and back
    assert H.codec_table8(ONES).tolist() == ONES.tolist() and int(H.codec_table8(TOP)[0, 0]) == 256
    for bad in (0, 65536, -1):
        with pytest.raises(ValueError):
            H.codec_table(bad)


def test_block_codec_refusals():
    x = np.zeros((8, 8), np.uint16)
    for bad in (np.zeros((8, 8), np.int64), np.full((8, 8), 65536), np.ones((8, 7), np.int64), np.ones((8, 8)), None):
        with pytest.raises(ValueError):
            H.block_codec(x, bad)
    for bad in ((8, 0), (0, -1), (0,), 3):
        with pytest.raises(ValueError):
            H.block_codec(x, ONES, bad)
    for bad in (np.zeros((8, 9), np.uint16), np.zeros((8, 8), np.int32), np.zeros((0, 0), np.uint16), np.zeros(8, np.uint16)):
        with pytest.raises(ValueError):
            H.block_codec(bad, ONES)


SIDE = 96
STUDY = dict(shutters=[10], translations=[12], rotations=[9], sigmas=[16.0], factors=[0.05], blurs=(2,))


def _study(**kw):
    return H.run_study(phantom(SIDE, 4, noise=4.0), StubRunner(SIDE), rng=np.random.default_rng(2), **STUDY, **kw)


def test_run_study_codec_rows():
    plain, coded = _study(), _study(codecs=(16, 4096))
    assert [r["alteration"] for r in coded] == [r["alteration"] for r in plain] + ["codec_16", "codec_4096"]
    assert coded[:len(plain)] == plain                                # every other row is the row of the study without codecs
    assert _study(codecs=None) == plain and _study(codecs=()) == plain
    raw = phantom(SIDE, 4, noise=4.0)
    runner = StubRunner(SIDE)
    unalt = runner.run(raw)
    for row, s in zip(coded[len(plain):], (16, 4096)):
        assert set(row) == {"alteration", "direct", "registered", "mean_cnr"}
        t = H.codec_table(s)
        alt = runner.run(H.block_codec(raw, t))
        assert row["direct"] == H.similarities(alt, unalt)
        # compress-before against compress-after: the unaltered result through the 8-bit table on the raw plane's block grid
        assert row["registered"] == H.similarities(alt, H.block_codec(unalt, H.codec_table8(t), (H.PROCESSING_MARGIN % 8,) * 2))


def test_study_options_codecs_and_refusals():
    runner = StubRunner(SIDE)
    args = (SIDE, runner, [], [], [], [], [], None, None, False, 0, False, 0, 0, False, 0, False, None)
    assert H.study_options(*args).codecs == [] and H.study_options(*args, codecs=H.CODECS).codecs == list(H.CODECS)
    assert H.study_options(*args, codecs=(16,)).keys == H.study_options(*args).keys      # rows, not keys
    for bad in ((0,), (65536,), ("x",), 5):
        with pytest.raises(ValueError):
            H.study_options(*args, codecs=bad)
    with pytest.raises(ValueError):
        H.study_options(20, runner, [], [], [], [], [], None, None, False, 0, False, 0, 0, False, 0, False, None, codecs=(16,))
    import inspect
    assert inspect.signature(H.run_study).parameters["codecs"].default is None


def test_abi_names_the_calls():
    assert mp.ABI["musica_alter_codec"] == (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint16)])
    assert mp.ABI["musica_sim_codec_reference"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16), C.c_uint32])
    t = mp.codec_table_words([[1] * 8] * 8)
    assert t.dtype == np.uint16 and t.flags["C_CONTIGUOUS"] and t.shape == (8, 8)
    assert mp.OUT_MARGIN % 8 == H.PROCESSING_MARGIN % 8 == 2


def test_the_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "musica.h")).read()
    assert re.search(r"int musica_alter_codec\(musica_ctx\* ctx, uint32_t image_index, const uint16_t table\[64\]\);", text)
    assert re.search(r"int musica_sim_codec_reference\(musica_ctx\* ctx, uint32_t dst_slot, uint32_t src_slot, const uint16_t table\[64\], uint32_t origin\);", text)
    assert "#define MUSICA_ABI_VERSION 3" in text
    kernel = open(os.path.join(root, "metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd", "csrc", "kernels_codec.hip")).read()
    literals = re.search(r"constexpr int m\[8\]\[8\] = (\{.*?\});", kernel, re.S).group(1)
    assert [int(v) for v in re.findall(r"-?\d+", literals)] == [v for row in R.M for v in row]     # the device's 64 literals


def test_the_cli_takes_the_flags(capsys):
    with pytest.raises(SystemExit):
        H.main(["--codecs", "16,4096", "--lattice", "8", "--lut-tables", "--size", "160"])      # parsed, then refused for the other flag
    assert "--luts" in capsys.readouterr().err
    for bad in (["--codecs", "0"], ["--codecs", "16,x"], ["--lattice", "3"], ["--lattice", "64"]):
        with pytest.raises(SystemExit):
            H.main(bad + ["--size", "160"])
        capsys.readouterr()
    assert H.codec_list("16,64") == (16, 64)

"""harness.ensemble_statistics, the numpy restatement of musica_sim_ensemble_result (include/musica.h): the integer identity
K sq_err_sum == sq_bias_sum + var_sum, tiles that sum to the totals, the doubles against np.mean / np.var in f64, the degenerate
ensembles (K = 1, identical realisations), the extreme the u32 accumulators are sized for, and ensemble_stream's range."""
import math

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp

SIDE = 150
# (ax, ay, bx, by, w, h): ragged against the 64-pixel tiles, unequal offsets, a region under one tile, one of exactly two tiles
REGIONS = [(0, 0, 0, 0, SIDE, SIDE), (3, 5, 11, 2, 131, 67), (70, 1, 0, 80, 7, 7), (1, 1, 1, 1, 128, 64), (17, 9, 5, 20, 65, 129)]


def _stack(k, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(SIDE, SIDE))
    outs = np.clip(base[None] + rng.integers(-30, 31, size=(k, SIDE, SIDE)), 0, 255).astype(np.uint8)
    b = np.clip(base + rng.integers(-5, 6, size=(SIDE, SIDE)), 0, 255).astype(np.uint8)
    return outs, b


@pytest.mark.parametrize("k", [1, 2, 7])
@pytest.mark.parametrize("region", REGIONS)
def test_identity_tiles_and_moments(k, region):
    outs, b = _stack(k, 100 + k)
    r = H.ensemble_statistics(outs, b, region)
    ax, ay, bx, by, w, h = region
    n = w * h
    assert list(r) == list(H.ENSEMBLE_KEYS) + ["tile_tables"]
    assert all(isinstance(r[key], int) for key in mp.ENSEMBLE_INTEGERS) and all(isinstance(r[key], float) for key in mp.ENSEMBLE_METRICS)
    assert r["pixels"] == n and r["realisations"] == k and (r["tiles_x"], r["tiles_y"]) == ((w + 63) // 64, (h + 63) // 64)
    assert k * r["sq_err_sum"] == r["sq_bias_sum"] + r["var_sum"]
    tt = r["tile_tables"]
    assert tt.shape == (r["tiles_y"], r["tiles_x"], 2) and tt.dtype == np.uint64
    assert sum(int(v) for v in tt[..., 0].ravel()) == r["sq_bias_sum"] and sum(int(v) for v in tt[..., 1].ravel()) == r["var_sum"]
    # a tile's entry is the same query over the tile alone
    ty, tx = r["tiles_y"] - 1, r["tiles_x"] - 1
    tw, th = w - 64 * tx, h - 64 * ty
    if tw >= 7 and th >= 7:
        one = H.ensemble_statistics(outs, b, (ax + 64 * tx, ay + 64 * ty, bx + 64 * tx, by + 64 * ty, tw, th))
        assert (one["sq_bias_sum"], one["var_sum"]) == (int(tt[ty, tx, 0]), int(tt[ty, tx, 1]))
    a = outs[:, ay:ay + h, ax:ax + w].astype(np.float64)
    cb = b[by:by + h, bx:bx + w].astype(np.float64)
    mean = a.mean(axis=0)
    assert abs(r["mean_shift"] - np.mean(mean - cb)) <= 1e-9
    assert abs(r["bias_rms"] - math.sqrt(np.mean((mean - cb) ** 2))) <= 1e-9
    assert r["sq_err_sum"] == int(np.sum((outs[:, ay:ay + h, ax:ax + w].astype(np.int64) - b[by:by + h, bx:bx + w].astype(np.int64)) ** 2))
    assert abs(r["mse"] - (1.0 - math.sqrt(np.mean((a - cb[None]) ** 2)) / 255.0)) <= 1e-9
    assert r["abs_bias_max"] == int(round(k * np.abs(mean - cb).max()))
    assert 0.0 <= r["bias_fraction"] <= 1.0
    if k == 1:
        assert r["var_sum"] == 0 and r["var_max"] == 0 and r["noise_rms"] == 0.0
        assert r["bias_fraction"] == (1.0 if r["sq_bias_sum"] else 0.0)
    else:
        var = a.var(axis=0, ddof=1)
        assert abs(r["noise_rms"] - math.sqrt(np.mean(var))) <= 1e-9
        assert abs(r["var_max"] / (k * (k - 1)) - var.max()) <= 1e-9


@pytest.mark.parametrize("k", [1, 5])
def test_identical_realisations_equal_to_b_give_zeros(k):
    b = np.random.default_rng(3).integers(0, 256, size=(SIDE, SIDE), dtype=np.uint8)
    r = H.ensemble_statistics(np.stack([b] * k), b, (2, 3, 2, 3, 140, 71))
    for key in ("sq_bias_sum", "var_sum", "sq_err_sum", "bias_sum", "abs_bias_max", "var_max"):
        assert r[key] == 0, key
    assert r["mean_shift"] == 0.0 and r["bias_rms"] == 0.0 and r["noise_rms"] == 0.0
    assert r["mse"] == 1.0 and r["bias_fraction"] == 0.0
    assert not r["tile_tables"].any()


def test_extreme_1024_planes_of_255_against_0():
    k = mp.SIM_ENSEMBLE_MAX
    r = H.ensemble_statistics(np.full((k, 64, 64), 255, dtype=np.uint8), np.zeros((64, 64), dtype=np.uint8), (0, 0, 0, 0, 64, 64))
    assert k == 1024 and r["realisations"] == 1024 and r["pixels"] == 4096 and (r["tiles_x"], r["tiles_y"]) == (1, 1)
    assert r["abs_bias_max"] == 261120 and r["bias_sum"] == 261120 * 4096
    assert r["sq_bias_sum"] == 261120 ** 2 * 4096 and r["var_sum"] == 0 and r["var_max"] == 0
    assert r["sq_err_sum"] == 65025 * 1024 * 4096
    assert r["tile_tables"].tolist() == [[[261120 ** 2 * 4096, 0]]]
    assert r["mean_shift"] == 255.0 and r["bias_rms"] == 255.0 and r["noise_rms"] == 0.0 and r["mse"] == 0.0 and r["bias_fraction"] == 1.0


def test_refusals():
    outs, b = _stack(2, 9)
    for region in [(0, 0, 0, 0, 6, 50), (0, 0, 0, 0, 50, 6), (SIDE - 49, 0, 0, 0, 50, 50), (0, 0, 0, SIDE - 49, 50, 50), (-1, 0, 0, 0, 50, 50)]:
        with pytest.raises(ValueError):
            H.ensemble_statistics(outs, b, region)
    with pytest.raises(ValueError):
        H.ensemble_statistics(outs[:0], b, (0, 0, 0, 0, 50, 50))
    with pytest.raises(ValueError):
        H.ensemble_statistics(outs.astype(np.int32), b, (0, 0, 0, 0, 50, 50))
    with pytest.raises(ValueError):       # the integers of two different queries do not satisfy the identity
        H.ensemble_summary(10, 10, 3, 0, 1, 1, 5, 7, 7)


def test_ensemble_streams_never_meet_a_rows_own_stream():
    assert H.ensemble_stream(1, 0) == 1024 and H.ensemble_stream(1, 1023) == 2047 and H.ensemble_stream(2, 0) == 2048
    seen = set()
    for ordinal in range(1, 40):
        for j in range(mp.SIM_ENSEMBLE_MAX):
            s = H.ensemble_stream(ordinal, j)
            assert s >= 1024 and s == 1024 * ordinal + j and s not in seen
            seen.add(s)
    assert not seen & set(range(1, 1024))        # the rows' own streams are their ordinals
    for bad in [(0, 0), (1, 1024), (1, -1)]:
        with pytest.raises(ValueError):
            H.ensemble_stream(*bad)


def test_ensemble_maps_are_the_tile_rms():
    outs, b = _stack(7, 21)
    r = H.ensemble_statistics(outs, b, REGIONS[0])
    bias, noise = H.ensemble_maps(r["tile_tables"], SIDE, SIDE, 7)
    assert bias.shape == noise.shape == (3, 3) and bias.dtype == np.uint8
    one = H.ensemble_statistics(outs, b, (128, 64, 128, 64, SIDE - 128, 64))      # tile (1, 2)
    assert bias[1, 2] == int(round(one["bias_rms"])) and noise[1, 2] == int(round(one["noise_rms"]))

"""csrc/curve_lut.h's lookup for arguments that cannot be negative (musica_lut_eval_nonneg: the expand launches that compute sdev in
registers call it on what musica_rms25_8 returns) equals the general lookup (musica_lut_eval, pinned against the literal scan by
test_curve_lut_host.py) on its whole domain: every pattern with the sign bit clear and every NaN of either sign.

The stand-alone program tests/lut_nonneg_host.cpp compares the two bit for bit, for every noise mode maxBin = 1 .. 2048 and the
lowContrastFactors of test_curve_lut_host.py, at every critical point (abscissae and their neighbours, bucket edges, 0, the smallest
denormal, 1, the values around 2, +inf, the ends of both NaN ranges), and for every 64th noise mode over the domain in steps of 4099
patterns. Built plain and with -fsanitize=address,undefined (the program has its own main; nothing is preloaded)."""
import os
import re
import subprocess

import pytest

from test_curve_lut_host import CSRC, ROOT, _compiler, _lows

SRC = os.path.join(ROOT, "tests", "lut_nonneg_host.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_nonnegative_lookup_equals_the_general_lookup_on_its_domain(sanitize, tmp_path):
    exe = str(tmp_path / "lut_nonneg_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    cmd = [_compiler(), "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"] + flags + ["-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    lows = _lows()[:3] if sanitize else _lows()
    run = subprocess.run([exe] + lows, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    m = re.search(r"ok curves=(\d+) checks=(\d+)", run.stdout)
    assert m, run.stdout[-2000:]
    curves, checks = (int(g) for g in m.groups())
    assert curves == 2048 * len(lows)                                  # every noise mode has a table
    assert checks > 2048 * len(lows) * (33 * 3 + 16) + 32 * len(lows) * (2 ** 31 // 4099)   # critical points of every curve, the sweep of every 64th

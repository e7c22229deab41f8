"""A literal second restatement of metrics.block_codec and metrics.lattice_statistics, written with nested loops and Python ints: it
knows nothing of numpy's integer types, of padding, of reshapes or of bincounts. The tests hold the numpy statements to it. And the
stand-in pipeline that the host-path study tests of both restatements score with (StubRunner)."""
import math

import numpy as np

MARGIN = 10   # harness.PROCESSING_MARGIN: what the pipeline crops on every side

# M[0][x] = 512, M[u][x] = rint(512 sqrt 2 cos((2x + 1) u pi / 16)): the contract's 64 literals, typed here a second time
M = [[512, 512, 512, 512, 512, 512, 512, 512],
     [710, 602, 402, 141, -141, -402, -602, -710],
     [669, 277, -277, -669, -669, -277, 277, 669],
     [602, -141, -710, -402, 402, 710, 141, -602],
     [512, -512, -512, 512, 512, -512, -512, 512],
     [402, -710, 141, 602, -602, -141, 710, -402],
     [277, -669, 669, -277, -277, 669, -669, 277],
     [141, -402, 602, -710, 710, -602, 402, -141]]


def matrix_from_the_cosines():
    return [[512 if u == 0 else int(round(512 * math.sqrt(2) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)] for u in range(8)]


def rs(t, s):
    return (t + (1 << (s - 1))) >> s   # Python's >> of a negative int floors: the arithmetic shift


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def codec_block(X, Q, seen=None):
    """One 8 x 8 block X[y][x] of level-shifted pixels with the table Q[v][u]: X'[y][x] before the shift back. seen: a dict that
    collects the largest magnitude of every raw product and stage."""
    def note(name, v):
        if seen is not None:
            seen[name] = max(seen.get(name, 0), abs(v))
        return v

    A = [[rs(note("XMt", sum(X[y][x] * M[u][x] for x in range(8))), 10) for u in range(8)] for y in range(8)]
    F = [[note("F", rs(note("MA", sum(M[v][y] * A[y][u] for y in range(8))), 11)) for u in range(8)] for v in range(8)]
    Fq = [[0] * 8 for _ in range(8)]
    for v in range(8):
        for u in range(8):
            q = (abs(F[v][u]) + (Q[v][u] >> 1)) // Q[v][u]
            Fq[v][u] = note("Fq", (-q if F[v][u] < 0 else q) * Q[v][u])
    A2 = [[clamp(rs(note("MtF", sum(M[v][y] * Fq[v][u] for v in range(8))), 10), -(1 << 18), (1 << 18) - 1) for u in range(8)] for y in range(8)]
    return [[rs(note("A2M", sum(A2[y][u] * M[u][x] for u in range(8))), 11) for x in range(8)] for y in range(8)]


def block_codec(plane, table, origin=(0, 0), bits=16, seen=None):
    """plane: a list of n lists of n ints; table: 8 lists of 8 ints; returns the same shape."""
    n = len(plane)
    oy, ox = origin
    half, top = 1 << (bits - 1), (1 << bits) - 1
    out = [[None] * n for _ in range(n)]
    for gy in range(0, n + oy, 8):          # the grid's blocks; grid position g is plane position g - o
        for gx in range(0, n + ox, 8):
            X = [[plane[clamp(gy + y - oy, 0, n - 1)][clamp(gx + x - ox, 0, n - 1)] - half for x in range(8)] for y in range(8)]
            X2 = codec_block(X, table, seen)
            for y in range(8):
                for x in range(8):
                    py, px = gy + y - oy, gx + x - ox
                    if 0 <= py < n and 0 <= px < n:
                        out[py][px] = clamp(X2[y][x] + half, 0, top)
    return out


def lattice_statistics(a, b, region, period, origin):
    """One query: table[row phase][column phase][8] of Python ints."""
    ax, ay, bx, by, w, h = region
    t = [[[0] * 8 for _ in range(period)] for _ in range(period)]
    for j in range(h - 1):
        for i in range(w - 1):
            c = t[(ay + j + origin) % period][(ax + i + origin) % period]
            va, vb = a[ay + j][ax + i], b[by + j][bx + i]
            c[0] += 1
            c[1] += va
            c[2] += vb
            c[3] += (va - vb) ** 2
            c[4] += (a[ay + j][ax + i + 1] - va) ** 2
            c[5] += (b[by + j][bx + i + 1] - vb) ** 2
            c[6] += (a[ay + j + 1][ax + i] - va) ** 2
            c[7] += (b[by + j + 1][bx + i] - vb) ** 2
    return t


class StubRunner:
    """harness.Runner's interface with a stand-in for the pipeline: the cropped image's high byte."""

    def __init__(self, n):
        self.n = n
        self.proc = self
        self._last = None

    def run(self, raw, workdir=None):
        m = MARGIN
        self._last = (raw[m:-m, m:-m] >> 8).astype(np.uint8)
        return self._last

    def mean_cnr(self):
        return float(self._last.mean())

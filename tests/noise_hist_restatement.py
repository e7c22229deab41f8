"""A host restatement of the noise histogram's early-exit scan, and generators of inputs on which the early exit matters
(test infrastructure, next to golden_util.py). Plain numpy; nothing here comes from oracle/ or from the HIP sources.

THE SCAN (noise_hist.comp as DESIGN.md section 4 reads it). The pass over an sdev image of side S that belongs to an input of side N
is dispatched as N / 512 workgroups of 32 x 32 threads per axis, whatever the level: T = (N / 512) * 32 threads per axis. Thread
(gx, gy) owns the 16 x 16 area at (16 gx, 16 gy) and walks it with x outer and y inner. For every texel of a column it reads the
sdev value (a read outside the image gives 0) and leaves the COLUMN, not the area, at the first value that
    is == 0,   or   has value / 0.1f > 1,   or   lands in bin int(value / 0.1f * 2048 + 0.5f) == 0;
every other texel adds one to its bin, except that bin 2048 lies outside the histogram image: that add is dropped and the
column goes on. All arithmetic is binary32. The float -> int conversion truncates and gives 0 for a NaN (rule Q6 of the oracle's
hosting rules), so a NaN value is a bin-0 break; +inf is a `> 1` break. So a texel is counted only if every earlier row of its
(column, 16-row run) survived, and nothing at or beyond cov = 16 T = (N / 512) * 512 is ever read.

scan() returns the histogram, the per-texel "counted" map and, per (column, run) inside the image and the coverage, the row phase
and cause of the first break. coverage() turns such a record into the facts a test wants to hold about its INPUT (which phases,
causes, column residues, strip-edge lanes and row quarters the breaks fall on), so that a test can assert that its inputs still
decide what they were made to decide.

THE INPUTS. crafted_band() builds a band-pass plane whose 5 x 5 RMS sits in the counted range almost everywhere and carries a
lattice of small "killer" patches of the three kinds plus a few bin-2048 patches; crafted_raw() stamps a phantom's raw pixels with
rectangles, dither, checkers and a collimator frame for the tests that need a whole step."""
import numpy as np

AREA = 16                        # rows and columns of a thread's area
BINS = 2048
MAX_NOISE = np.float32(0.1)
GROUP_COVERAGE = 512             # 32 threads x 16 texels per workgroup and axis

NONE, ZERO, OVER, BIN0, BEYOND = 0, 1, 2, 3, 4
CAUSE_NAMES = {NONE: "none", ZERO: "== 0", OVER: "> 0.1", BIN0: "bin 0", BEYOND: "read beyond the image"}


def coverage_side(n):
    """Texels per axis that the dispatch of an input of side n reaches, at every level."""
    return (n // GROUP_COVERAGE) * GROUP_COVERAGE


def classify(cur):
    """Per value of a float32 array: (cause of a break or NONE, bin). What one trip of the inner loop decides."""
    cur = np.asarray(cur, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        adj = cur / MAX_NOISE
        t = adj * np.float32(BINS) + np.float32(0.5)
        assert adj.dtype == np.float32 and t.dtype == np.float32
        usable = np.isfinite(t) & (t < np.float32(2.0 ** 31))
        bins = np.where(usable, np.where(usable, t, np.float32(0)).astype(np.int64), 0)   # truncation; NaN -> 0 (Q6)
        cause = np.full(cur.shape, NONE, dtype=np.int8)
        zero = cur == 0
        over = ~zero & (adj > np.float32(1.0))
        cause[zero] = ZERO
        cause[over] = OVER
        cause[~zero & ~over & (bins == 0)] = BIN0
    return cause, bins


def scan(sdev, n):
    """The scan of one sdev plane (S x S, float32) of an input of side n.

    Returns (hist, counted, phase, cause):
      hist     uint32[2048];
      counted  bool[S, S], the texels that added to a bin or would have but for bin 2048;
      phase    int8[R, C] for the R = ceil(min(S, cov) / 16) runs and C = min(S, cov) columns inside image and coverage: the row
               phase 0 .. 15 of the column-run's first break, -1 where all 16 rows survive;
      cause    int8[R, C]: ZERO / OVER / BIN0, BEYOND where the first break is a read below the image's last row, NONE.
    Threads whose area starts outside the image read 0 at once and are left out."""
    sdev = np.asarray(sdev)
    assert sdev.dtype == np.float32 and sdev.ndim == 2 and sdev.shape[0] == sdev.shape[1]
    S = sdev.shape[0]
    cov = coverage_side(n)
    T = min(cov // AREA, -(-S // AREA))          # threads per axis whose area starts inside the image
    C = min(S, cov)
    hist = np.zeros(BINS, dtype=np.int64)
    counted = np.zeros((S, S), dtype=bool)
    phase = np.full((T, T * AREA), -1, dtype=np.int8)
    cause = np.zeros((T, T * AREA), dtype=np.int8)
    if T == 0:
        return hist.astype(np.uint32), counted, phase[:, :C], cause[:, :C]
    P = T * AREA
    padded = np.zeros((P, P), dtype=np.float32)   # a read outside the image gives 0
    padded[:min(S, P), :min(S, P)] = sdev[:min(S, P), :min(S, P)]
    inside = np.zeros((P, P), dtype=bool)
    inside[:min(S, P), :min(S, P)] = True
    counted_p = np.zeros((P, P), dtype=bool)
    for m in range(AREA):                          # x outer
        live = np.ones((T, T), dtype=bool)         # [gy, gx]: this column of the thread's area has not broken yet
        for k in range(AREA):                      # y inner
            cur = padded[k::AREA, m::AREA]
            why, bins = classify(cur)
            why = np.where(inside[k::AREA, m::AREA], why, BEYOND).astype(np.int8)
            first = live & (why != NONE)
            phase[:, m::AREA][first] = k
            cause[:, m::AREA][first] = why[first]
            live &= why == NONE
            counted_p[k::AREA, m::AREA] = live
            add = live & (bins < BINS)             # bin 2048: dropped, the column goes on
            hist += np.bincount(bins[add], minlength=BINS)
    counted[:min(S, P), :min(S, P)] = counted_p[:min(S, P), :min(S, P)]
    return hist.astype(np.uint32), counted, phase[:, :C], cause[:, :C]


def first_difference(sdev, n, got_hist):
    """Words for an assertion message: where a histogram that differs from scan()'s could have gone wrong. Names the bins that differ
    and, for the first of them, the first column-run with a break that holds a texel of that bin (level is the caller's to add)."""
    want, counted, phase, cause = scan(sdev, n)
    got_hist = np.asarray(got_hist).astype(np.int64)
    diff = np.flatnonzero(got_hist != want.astype(np.int64))
    if len(diff) == 0:
        return "histograms equal"
    b = int(diff[0])
    _, bins = classify(sdev)
    msg = "%d bins differ, first bin %d: got %d, restatement %d" % (len(diff), b, got_hist[b], want[b])
    C = phase.shape[1]
    ys, xs = np.nonzero(bins[:phase.shape[0] * AREA, :C] == b)
    for y, x in zip(ys, xs):
        r = y // AREA
        if phase[r, x] >= 0:
            return msg + "; first broken run holding that bin: column %d (x %% 8 = %d, lane %d of strip %d), run %d (rows %d..), first break at phase %d (%s), texel (x=%d, y=%d) is %scounted" % (
                x, x % 8, (x % 512) // 8, x // 512, r, r * AREA, phase[r, x], CAUSE_NAMES[int(cause[r, x])], x, y, "" if counted[y, x] else "not ")
    return msg + "; no broken run holds that bin"


def coverage(sdev, n):
    """What the breaks of one sdev plane decide. A dict:
      phases     set of first-break phases over all column-runs, -1 = a run without a break;
      causes     set of first-break causes among ZERO, OVER, BIN0 (BEYOND is listed under beyond);
      residues   set of x % 8 over the columns with a ZERO / OVER / BIN0 first break;
      lane0, lane63   such a break in a column with x % 512 < 8 / >= 504;
      has_lane63      the image and the coverage hold such a column at all;
      quarters   set of q = 0 .. 3: some run's first break falls in rows 4q .. 4q + 3 and every later quarter of that run holds a
                 texel that would be counted if the run were alive;
      dead_then_live  runs whose first break is at phase < 15 and that hold a live-looking texel afterwards;
      last_row, row0_then_live   runs that die in their last row / in row 0 with live-looking texels afterwards;
      revivals   column-runs that are broken and are followed, in the same column, by a run whose row 0 is counted;
      bin2048    counted texels whose bin is 2048;  occupied   bins with a count;  beyond   runs ended by the image's last row;
      runs       number of column-runs looked at."""
    hist, counted, phase, cause = scan(sdev, n)
    R, C = phase.shape
    why, bins = classify(sdev)
    own = np.zeros((R * AREA, C), dtype=bool)       # live-looking: the texel's own value would be counted
    rows = min(R * AREA, sdev.shape[0])
    own[:rows] = why[:rows, :C] == NONE
    own = own.reshape(R, AREA, C)
    real = (cause == ZERO) | (cause == OVER) | (cause == BIN0)
    k = np.arange(AREA)[None, :, None]
    after = own & (k > phase[:, None, :])
    later_q = [after[:, 4 * q:4 * q + 4].any(axis=1) for q in range(4)]
    quarters = set()
    for q in range(4):
        ok = real & (phase // 4 == q)
        for q2 in range(q + 1, 4):
            ok &= later_q[q2]
        if ok.any():
            quarters.add(q)
    live_after = after.any(axis=1)
    row0_counted = np.zeros((R, C), dtype=bool)
    row0_counted[:, :] = counted[:R * AREA:AREA, :C][:R]
    xs = np.arange(C)
    lane0_cols, lane63_cols = (xs % 512) < 8, (xs % 512) >= 504
    return {
        "phases": set(int(p) for p in np.unique(phase)),
        "causes": set(int(c) for c in np.unique(cause[real])),
        "residues": set(int(r) for r in np.unique(xs[real.any(axis=0)] % 8)),
        "lane0": bool(real[:, lane0_cols].any()),
        "lane63": bool(real[:, lane63_cols].any()),
        "has_lane63": bool(lane63_cols.any()),
        "quarters": quarters,
        "dead_then_live": int((real & (phase < 15) & live_after).sum()),
        "last_row": int((real & (phase == 15)).sum()),
        "row0_then_live": int((real & (phase == 0) & live_after).sum()),
        "revivals": int((real[:-1] & row0_counted[1:]).sum()) if R > 1 else 0,
        "bin2048": int((counted & (bins == BINS)).sum()),
        "occupied": int((hist != 0).sum()),
        "beyond": int((cause == BEYOND).sum()),
        "runs": int(R * C),
    }


def full_coverage_problems(cov, run_form=True):
    """The condition the crafted band planes are held to (a list of what is missing; empty = met): all 16 first-break phases and a
    run without a break, all three causes, all 8 column residues, a break in a lane-0 column and, where the plane has one inside the
    coverage, in a lane-63 column, first breaks in all four row quarters with live-looking texels in every later quarter, runs that
    die in their last row and in row 0 with live texels behind, a revival at y % 16 == 0, a bin-2048 texel and 30 occupied bins."""
    bad = []
    if cov["phases"] != set(range(-1, 16)):
        bad.append("phases %s" % sorted(cov["phases"]))
    if cov["causes"] != {ZERO, OVER, BIN0}:
        bad.append("causes %s" % sorted(cov["causes"]))
    if cov["residues"] != set(range(8)):
        bad.append("residues %s" % sorted(cov["residues"]))
    if not cov["lane0"]:
        bad.append("no break in a lane-0 column")
    if cov["has_lane63"] and not cov["lane63"]:
        bad.append("no break in a lane-63 column")
    if run_form and cov["quarters"] != {0, 1, 2, 3}:
        bad.append("quarters %s" % sorted(cov["quarters"]))
    for key in ("last_row", "row0_then_live", "revivals", "bin2048"):
        if cov[key] < 1:
            bad.append("no %s" % key)
    if cov["occupied"] < 30:
        bad.append("%d occupied bins" % cov["occupied"])
    return bad


def raw_coverage_problems(cov, level):
    """The condition the crafted raw images are held to, on the sdev image of `level`: levels 0 and 1 all 16 first-break phases, two of
    the three causes and all 8 column residues; levels 2 and 3 at least 8 phases."""
    bad = []
    phases = cov["phases"] - {-1}
    if level <= 1:
        if phases != set(range(16)):
            bad.append("phases %s" % sorted(phases))
        if len(cov["causes"]) < 2:
            bad.append("causes %s" % sorted(cov["causes"]))
        if cov["residues"] != set(range(8)):
            bad.append("residues %s" % sorted(cov["residues"]))
    elif len(phases) < 8:
        bad.append("phases %s" % sorted(phases))
    return bad


# ---- crafted band planes ------------------------------------------------------------------------------------------------------------
PATCH_PITCH_X = 9     # one more than a lane's 8 columns: the column residue mod 8 advances by one from patch to patch
ROW_STEP, ROW0 = 7, 3   # row offset of lattice column i: (7 i) % 16 + 3 (chosen so that a 65-texel level still shows every phase)
PATCH_PITCH_Y = 17    # one more than a run: the row phase advances by one from patch to patch


def crafted_band(side, seed, nonfinite=False):
    """A float32 band plane of side `side`, deterministic in (side, seed).

    Base: Gaussian noise whose amplitude rises along the diagonal from 1.5e-3 to 4.5e-3, so the 5 x 5 RMS (about the amplitude, give
    or take a seventh) spreads over bins 25 .. 110 and is never 0, never above 0.1.
    Lattice: patch (i, j) has its first dead texel row at ty = (7 i) % 16 + 17 j + 3 and its first dead column at tx = 1 + 9 i, so
    along j the row phase advances by one, along i the column residue mod 8 advances by one and the row phase by seven; the lattice
    runs over the whole plane and so crosses every strip edge (x % 512 in [504, 512) and [0, 8)). The kind cycles with i + j:
      0  exact zeros over (d + 4)^2 samples, d = 1 .. 3: d x d texels of sdev == 0;
      1  one sample of 5.0: sdev >= 1 over its 5 x 5 neighbourhood;
      2  samples of +-1e-5 over (d + 4)^2: d x d texels of sdev 1e-5 < 0.1 * 0.5 / 2048, bin 0.
    In every fourth lattice column the patches of odd j are bin-2048 patches instead: samples of
    amplitude 5e-4 over 9 x 9 (counted, bins around 10) and a centre sample of 0.49994, so the 25 texels around it have
    sdev^2 * 25 in 0.24994 + [0, 1e-5], inside [0.1 * 2047.5 / 2048, 0.1]^2 * 25 = [0.249878, 0.25]: bin 2048, dropped, the run goes on.
    nonfinite: one band sample becomes +inf (its 25 sdev texels are +inf: a `> 1` break) and one NaN (25 NaN texels: bin 0 by Q6)."""
    rng = np.random.default_rng([int(seed), int(side)])
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float32)
    amp = np.float32(1.5e-3) * (1 + 2 * (xx + yy) / np.float32(2 * side))
    band = (rng.standard_normal((side, side), dtype=np.float32) * amp).astype(np.float32)

    def block(x0, y0, w, h):
        return slice(max(y0, 0), max(min(y0 + h, side), 0)), slice(max(x0, 0), max(min(x0 + w, side), 0))

    i = 0
    while 1 + PATCH_PITCH_X * i < side:
        tx = 1 + PATCH_PITCH_X * i
        j = 0
        while (ROW_STEP * i) % 16 + PATCH_PITCH_Y * j + ROW0 < side:
            ty = (ROW_STEP * i) % 16 + PATCH_PITCH_Y * j + ROW0
            kind, d = (i + j) % 3, 1 + (i + 2 * j) % 3
            if kind == 1 and (tx + 2 >= side or ty + 2 >= side):
                kind = 0                                           # the large sample would fall outside: zeros instead
            if kind == 0:
                band[block(tx - 2, ty - 2, d + 4, d + 4)] = 0
            elif kind == 1:
                band[ty + 2, tx + 2] = 5.0
            else:
                s = block(tx - 2, ty - 2, d + 4, d + 4)
                band[s] = np.where(rng.random(band[s].shape) < 0.5, np.float32(-1e-5), np.float32(1e-5))
            j += 1
        i += 1
    # bin-2048 patches, written last: in every fourth lattice column they take the place of the patches of odd j (the 9 x 9 block
    # around the patch's centre covers that patch and stays clear of its neighbours, 9 columns and 17 rows away)
    i = 3
    while 1 + PATCH_PITCH_X * i + 4 < side:
        cx = 1 + PATCH_PITCH_X * i + 2
        j = 1
        while (ROW_STEP * i) % 16 + PATCH_PITCH_Y * j + ROW0 + 4 < side:
            cy = (ROW_STEP * i) % 16 + PATCH_PITCH_Y * j + ROW0 + 2
            s = block(cx - 4, cy - 4, 9, 9)
            band[s] = (rng.standard_normal(band[s].shape, dtype=np.float32) * np.float32(5e-4)).astype(np.float32)
            band[cy, cx] = np.float32(0.49994)
            j += 2
        i += 4
    if nonfinite and side >= 40:
        band[side // 2 + 3, 4] = np.inf
        band[side // 2 + 3 + PATCH_PITCH_Y, side - 5] = np.nan
    return band


# ---- crafted raw images ---------------------------------------------------------------------------------------------------------------
def crafted_raw(base, seed):
    """`base` (uint16, N x N, a phantom) stamped so that the sdev images of levels 0 .. 3 of its pyramid hold breaks at many row phases.
    The stamps lie on a grid of pitch 131 x 139 whose cell (i, j) starts at (20 + 131 i + j, 16 + 139 j + i): from cell to cell the
    stamps drift by one pixel in both axes. The stamp of a cell has edges that are no multiples of 16 and cycles through
      constant rectangles (value 0, 20000 or 65535) of 101 x 111, large enough to leave exact or near zeros of sdev down to level 3,
      rectangles of +-1 count dither on 12000: a band of 1e-5 or less, so bin 0,
      checkers of 0 / 65535 with cells of 1, 2, 4 or 8 pixels: sdev far above 0.1 at the level whose texel is a cell,
      smaller constant rectangles of 37 x 43 for levels 0 and 1;
    then a collimator frame of 21 black pixels left and top, 27 right and bottom."""
    img = np.array(base, dtype=np.uint16, copy=True)
    n = img.shape[0]
    rng = np.random.default_rng([int(seed), n])
    j = 0
    while 16 + 139 * j < n:
        i = 0
        while 20 + 131 * i < n:
            x0, y0 = 20 + 131 * i + j, 16 + 139 * j + i
            kind = (i + 2 * j) % 6
            if kind in (0, 3):
                img[y0:y0 + 111, x0:x0 + 101] = (0, 20000, 65535)[(i + j) % 3]
            elif kind == 1:
                s = img[y0:y0 + 90, x0:x0 + 77]
                s[...] = 12000 + rng.integers(-1, 2, size=s.shape)
            elif kind in (2, 5):
                c = 1 << ((i + j) % 4)
                s = img[y0:y0 + 96, x0:x0 + 88]
                ys, xs = np.mgrid[0:s.shape[0], 0:s.shape[1]]
                s[...] = np.where(((ys // c) + (xs // c)) % 2 == 0, 0, 65535)
            else:
                img[y0:y0 + 43, x0:x0 + 37] = (0, 65535)[i % 2]
            i += 1
        j += 1
    img[:21, :] = 0
    img[:, :21] = 0
    img[n - 27:, :] = 0
    img[:, n - 27:] = 0
    return img


# ---- the inputs the tests share -----------------------------------------------------------------------------------------------------
def level_side(n, level):
    """Side of pyramid level `level` of an input of side n (each level is half the one before, rounded up)."""
    for _ in range(level):
        n = (n + 1) // 2
    return n


def crafted_bands(n, k, nonfinite=False):
    """The crafted band planes of levels 0 .. 3 for batch member k of an input of side n."""
    return [crafted_band(level_side(n, i), 100 * k + i, nonfinite=nonfinite) for i in range(4)]

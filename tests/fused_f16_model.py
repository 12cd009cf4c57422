"""The arithmetic of SRCNN_MODE_FAST_F16 (k_fused_f16 and its host packer build_fused_f16_weights), restated in numpy float64
from the statement in DESIGN.md section 3, and the inputs on which that statement fixes every bit of the kernel's output.

The statement leaves the order of every sum open ("the order inside a 16-deep fp16 MFMA is not specified").  The order matters
only where a sum rounds.  If every term of a sum and the C operand that opens it are integer multiples of a power of two q, and
the sum of their magnitudes stays below 2^24 q, every partial sum in every order is a multiple of q below 2^24 q: exactly
representable in fp32.  No order can be observed then, and the kernel's output is determined bit for bit.  model() evaluates the
statement in float64 (exact on such inputs, whatever order numpy takes), checks every sum to be exactly representable in fp32
and reports how far inside that condition each layer stays.

  plain(up, blob)            the three-layer network with no split at all, written from the layer definitions
  model(up, blob, drop=())   the statement; drop names terms to omit or defects to plant (MUTATIONS), for the mutation check
  cases()                    the weight sets and planes tests/test_gpu_fused_f16_exact.py runs, seeded

Blob order (8129 floats): b1[64], W1[64][9][9] as [k][row][col], b2[32], W2[32][64] as [m][c], b3, W3[32][5][5] as [m][x][y]
(x = column offset: the oracle's order, src/libsrcnn.cpp:512).
"""
import numpy as np

F_INV = 2.0 ** -8
F16_MIN_NORMAL = 2.0 ** -14
BLOB = 8129
# what model(drop=...) understands: a lo piece left out, a tap left out, taps / channels exchanged, W3 read untransposed, and the
# two border defects (zero padding of Y in place of clamp-to-edge; layer-2 activations outside the image computed from a clamped
# window -- what a gather clamped at the wave's tile and not at the image reads -- in place of clamp-to-edge of the activations)
MUTATIONS = ("yl", "w1l", "c1l", "w2l", "c2l", "w3l", "tap88", "swap_taps", "swap_channels", "w3_yx", "zero_pad", "tile_clamp")
BORDER_MUTATIONS = ("zero_pad", "tile_clamp")
SWAPPED_CHANNELS = (5, 41)          # layer-2 input channels exchanged by "swap_channels": one of each 32-channel block


def unpack(blob):
    b = np.ascontiguousarray(blob, np.float32)
    assert b.shape == (BLOB,), b.shape
    o = np.cumsum([0, 64, 64 * 81, 32, 32 * 64, 1, 32 * 25])
    return (b[o[0]:o[1]], b[o[1]:o[2]].reshape(64, 9, 9), b[o[2]:o[3]], b[o[3]:o[4]].reshape(32, 64), b[o[4]],
            b[o[5]:o[6]].reshape(32, 5, 5))


def pack(b1, w1, b2, w2, b3, w3):
    blob = np.concatenate([np.ravel(np.asarray(a, np.float64)) for a in (b1, w1, b2, w2, [b3], w3)]).astype(np.float32)
    assert blob.shape == (BLOB,)
    return blob


def split(x):
    """split(x) = (hi, lo): hi = f16(x), lo = f16(x - (float)hi), round to nearest even; x fp32, the pieces returned as float64."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def lowbit(a):
    """The largest power of two that divides every non-zero element of a (inf if there is none)."""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = np.unique(a[a != 0])
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    mant = (m * 2.0 ** 53).astype(np.int64)
    return float(np.ldexp((mant & -mant).astype(np.float64), e - 53).min())


def _in_fp32(a):
    """Number of elements of the float64 array that are not exactly representable in fp32."""
    with np.errstate(over="ignore"):
        return int(np.count_nonzero(a.astype(np.float32).astype(np.float64) != a))


def _sum2(a, b):
    """a + b in float64 and the number of elements where that addition itself rounded (Knuth's two-sum)."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    return s, int(np.count_nonzero(err))


def _windows(img, rows, cols, n, zero_pad=False):
    """out[i, j, dy, dx] = img[rows[i] + dy - n // 2, cols[j] + dx - n // 2], clamped to the edge (or zero outside)."""
    h, w = img.shape
    ry = rows[:, None] + np.arange(n)[None, :] - n // 2
    cx = cols[:, None] + np.arange(n)[None, :] - n // 2
    out = img[np.clip(ry, 0, h - 1)[:, None, :, None], np.clip(cx, 0, w - 1)[None, :, None, :]]
    if zero_pad:
        inside = ((ry >= 0) & (ry < h))[:, None, :, None] & ((cx >= 0) & (cx < w))[None, :, None, :]
        out = np.where(inside, out, 0.0)
    return out


class Inexact(AssertionError):
    pass


def _layer(name, report, x_hi, x_lo, w_hi, w_lo, c, exact, drop_x, drop_w):
    """C + sum_k (wh xh + wh xl + wl xh) for pieces x (N, K), w (M, K) and the C operand c (N, M) or (M,): the fp32 value of the
    sum, with the layer's entry of the report filled in."""
    if drop_x:
        x_lo = np.zeros_like(x_lo)
    if drop_w:
        w_lo = np.zeros_like(w_lo)
    s = x_hi @ w_hi.T + x_lo @ w_hi.T + x_hi @ w_lo.T + c
    mag = np.abs(x_hi) @ np.abs(w_hi).T + np.abs(x_lo) @ np.abs(w_hi).T + np.abs(x_hi) @ np.abs(w_lo).T + np.abs(c)
    # q: per operand index k every term is a multiple of lowbit(w[:, k]) * lowbit(x[:, k]); C has its own
    q = lowbit(c)
    for k in range(x_hi.shape[1]):
        qw, qx = lowbit(np.stack([w_hi[:, k], w_lo[:, k]])), lowbit(np.stack([x_hi[:, k], x_lo[:, k]]))
        if np.isfinite(qw) and np.isfinite(qx):
            q = min(q, qw * qx)
    bad = _in_fp32(s)
    report[name] = dict(budget=float(mag.max() / q) if np.isfinite(q) else 0.0, q=q, inexact=bad)
    if exact and bad:
        raise Inexact("%s: %d sums are not exactly representable in fp32" % (name, bad))
    return s.astype(np.float32)


def _subnormal(*pieces):
    return sum(int(np.count_nonzero((p != 0) & (np.abs(p) < F16_MIN_NORMAL))) for p in pieces)


def _share(lo, of=None):
    """Share of the operands whose lo piece is non-zero: of all samples (activations, Y), or of the non-zero weights."""
    n = lo.size if of is None else int(np.count_nonzero(of))
    return float(np.count_nonzero(lo)) / max(n, 1)


def model(up, blob, drop=(), exact=True):
    """(Y', report) of the statement for the upscaled plane `up` (h, w) and the weight blob.  exact: raise Inexact unless every
    sum is exactly representable in fp32 (off: the sums are rounded to fp32 once, for real weights).  report: per sum ("l1",
    "l2", "p", "gather") budget = max over the plane of (sum|terms| + |C|) / q, q and inexact; "subnormal": non-zero fp16
    subnormal pieces; "lo": share of non-zero lo pieces per operand (Y, c1, c2: of all samples; W1, W2, W3: of the non-zero
    weights); "clamped": share of output samples on 0 or 255; "final_inexact": outputs whose last fmaf rounded."""
    drop = (drop,) if isinstance(drop, str) else tuple(drop)
    assert all(d in MUTATIONS for d in drop), drop
    up = np.ascontiguousarray(up, np.float32)
    h, w = up.shape
    b1, w1, b2, w2, b3, w3 = unpack(blob)
    report = {}
    # layer-2 positions: the image's, or (tile_clamp) the image's +-2 with nothing clamped but the window of Y
    ext = 2 if "tile_clamp" in drop else 0
    rows, cols = np.arange(-ext, h + ext), np.arange(-ext, w + ext)
    n = rows.size * cols.size

    # ---- layer 1 ----
    yh, yl = split(up)
    if "yl" in drop:
        yl = np.zeros_like(yl)
    w1 = w1.copy()
    if "swap_taps" in drop:
        w1[:, 0, 8], w1[:, 8, 0] = w1[:, 8, 0].copy(), w1[:, 0, 8].copy()
    w1s = (w1 * np.float32(256.0)).reshape(64, 81)
    w1h, w1l = split(w1s)
    ph = _windows(yh, rows, cols, 9, "zero_pad" in drop).reshape(n, 81)
    pl = _windows(yl, rows, cols, 9, "zero_pad" in drop).reshape(n, 81)
    # the chain opener: fmaf(256 w1[k][8][8] (unsplit), (float)yh + (float)yl, 256 b1[k])
    y88 = (ph[:, 80].astype(np.float32) + pl[:, 80].astype(np.float32)).astype(np.float64)
    w88 = np.zeros(64) if "tap88" in drop else w1s[:, 80].astype(np.float64)
    opener, rounded = _sum2(y88[:, None] * w88[None, :], (b1 * np.float32(256.0)).astype(np.float64)[None, :])
    bad = rounded + _in_fp32(opener)
    if exact and bad:
        raise Inexact("l1: %d chain openers are not exactly representable in fp32" % bad)
    opener = opener.astype(np.float32).astype(np.float64)
    w1h[:, 80] = 0.0
    w1l[:, 80] = 0.0
    a1 = _layer("l1", report, ph, pl, w1h, w1l, opener, exact, False, "w1l" in drop)
    report["l1"]["inexact"] += bad
    if w88.any() and y88.any():
        report["l1"]["q"] = min(report["l1"]["q"], lowbit(w88) * lowbit(y88))       # (the budget already counts |opener|)
    c1 = np.maximum(a1 * np.float32(F_INV), np.float32(0.0))

    # ---- layer 2 ----
    c1h, c1l = split(c1)
    w2 = w2.copy()
    if "swap_channels" in drop:
        a, b = SWAPPED_CHANNELS
        w2[:, a], w2[:, b] = w2[:, b].copy(), w2[:, a].copy()
    w2h, w2l = split(w2 * np.float32(256.0))
    a2 = _layer("l2", report, c1h, c1l, w2h, w2l, (b2 * np.float32(256.0)).astype(np.float64), exact, "c1l" in drop, "w2l" in drop)
    c2 = np.maximum(a2 * np.float32(F_INV), np.float32(0.0))

    # ---- layer 3: 25 outputs per position, then the shifted gather ----
    c2h, c2l = split(c2)
    w3t = w3 if "w3_yx" in drop else w3.transpose(0, 2, 1)               # [m][x][y] -> [m][dy][dx]
    w3h, w3l = split((w3t * np.float32(256.0)).reshape(32, 25).T)       # (25, 32)
    p = _layer("p", report, c2h, c2l, w3h, w3l, np.zeros(25), exact, "c2l" in drop, "w3l" in drop)
    p = p.astype(np.float64).reshape(rows.size, cols.size, 5, 5)
    oy, ox = np.arange(h), np.arange(w)
    if not ext:          # clamp-to-edge of the activations is clamp-to-edge of P
        iy = np.clip(oy[:, None] + np.arange(5)[None, :] - 2, 0, h - 1)
        ix = np.clip(ox[:, None] + np.arange(5)[None, :] - 2, 0, w - 1)
    else:
        iy = oy[:, None] + np.arange(5)[None, :]
        ix = ox[:, None] + np.arange(5)[None, :]
    o = np.zeros((h, w))
    mag = np.zeros((h, w))
    for dy in range(5):
        for dx in range(5):
            t = p[iy[:, dy][:, None], ix[:, dx][None, :], dy, dx]
            o += t
            mag += np.abs(t)
    q = lowbit(p)
    bad = _in_fp32(o)
    report["gather"] = dict(budget=float(mag.max() / q) if np.isfinite(q) else 0.0, q=q, inexact=bad)
    if exact and bad:
        raise Inexact("gather: %d sums are not exactly representable in fp32" % bad)
    o = o.astype(np.float32).astype(np.float64)
    y, rounded = _sum2(o * F_INV, np.full_like(o, np.float64(b3)))
    report["final_inexact"] = rounded + _in_fp32(y)
    out = np.minimum(np.maximum(y.astype(np.float32), np.float32(0.0)), np.float32(255.0))

    report["subnormal"] = _subnormal(yh, yl, w1h, w1l, c1h, c1l, w2h, w2l, c2h, c2l, w3h, w3l)
    report["lo"] = dict(Y=_share(yl), W1=_share(w1l, w1h), c1=_share(c1l), W2=_share(w2l, w2h), c2=_share(c2l), W3=_share(w3l, w3h))
    report["clamped"] = float(np.count_nonzero((out == 0) | (out == 255))) / out.size
    return out, report


def plain(up, blob):
    """The network as its layers are defined, in float64 with no split: c1 = relu(b1 + W1 * Y) with Y clamped to the edge,
    c2 = relu(b2 + W2 c1), Y' = clamp(b3 + W3 * c2, 0, 255) with the ACTIVATIONS clamped to the edge, rounded to fp32 at the end."""
    up = np.asarray(up, np.float64)
    h, w = up.shape
    b1, w1, b2, w2, b3, w3 = (np.asarray(a, np.float64) for a in unpack(blob))

    def shifted(a, dy, dx):      # a[..., y + dy, x + dx], clamped to the edge
        ys = np.clip(np.arange(h) + dy, 0, h - 1)
        xs = np.clip(np.arange(w) + dx, 0, w - 1)
        return a[..., ys[:, None], xs[None, :]]

    c1 = np.zeros((64, h, w)) + b1[:, None, None]
    for i in range(9):
        for j in range(9):
            c1 += w1[:, i, j][:, None, None] * shifted(up, i - 4, j - 4)[None]
    c1 = np.maximum(c1, 0.0)
    c2 = np.maximum(np.tensordot(w2, c1, axes=(1, 0)) + b2[:, None, None], 0.0)
    out = np.full((h, w), float(b3))
    for x in range(5):
        for y in range(5):
            out += np.tensordot(w3[:, x, y], shifted(c2, y - 2, x - 2), axes=(0, 0))
    return np.minimum(np.maximum(out, 0.0), 255.0).astype(np.float32)


# ---- the cases ------------------------------------------------------------------------------------------------------------
# upscaled-plane shapes (h, w): one sample, one row, one column, one ragged wave strip, a wave strip to the column and one past
# it, three strips over ten ring stages, several chunks of at least 16 rows with a workgroup strip plus three columns, and two
# workgroup strips plus one column
SHAPES = [(1, 1), (1, 33), (33, 1), (5, 59), (20, 60), (20, 61), (37, 130), (66, 483), (3, 961)]
WIDE_SHAPES = [(5, 59), (20, 61), (37, 130)]
BAND_SHAPE = (66, 130)
SEED = 20261021


def _signed(rng, top, size):
    """Non-zero integers of [-top, top], every value about equally often."""
    return rng.integers(1, top + 1, size) * rng.choice([-1, 1], size)


def _wide(rng, size):
    """+-(2048 + odd): twelve significant bits, so split() leaves a lo piece of +-1 (in units of the value's last bit)."""
    return (2049 + 2 * rng.integers(0, 1024, size)) * rng.choice([-1, 1], size)


def _one_negative(top):
    """values(rng, n) for _rows_of: integers of [1, top], the last one negated -- a row of W2 or W3 whose inputs are activations
    (never negative) then gives sums of either sign, and its ReLU output is positive on a good share of the samples."""
    def values(rng, n):
        v = rng.integers(1, top + 1, n)
        v[-1] = -v[-1]
        return v
    return values


def _rows_of(rng, rows, cols, per_row, values, among=None):
    """(rows, cols) of zeros but for per_row entries of every row, at columns drawn from `among`, filled by values(rng, n)."""
    w = np.zeros((rows, cols))
    among = np.arange(cols) if among is None else np.asarray(among)
    for r in w:
        r[rng.choice(among, per_row, replace=False)] = values(rng, per_row)
    return w


def _single_tap(rng, w1, channels):
    """Channels of W1 that pass one sample of Y on: weight 1 on one tap (a different one per channel), 0 elsewhere."""
    for k in channels:
        w1[k] = 0
        w1[k].reshape(81)[rng.integers(0, 81)] = 1
    return w1


def _w3_one_channel(rng, taps):
    """W3[m][x][y] of zeros but for one weight of +-1 on each of `taps` taps, every tap on a layer-2 channel of its own: with one
    channel per tap the gather's budget is spent on observing as many layer-2 channels as there are taps."""
    w3 = np.zeros((32, 5, 5))
    for t, m in zip(rng.choice(25, taps, replace=False), rng.permutation(32)):
        w3[m, t // 5, t % 5] = rng.choice([-1, 1])
    return w3


def _w3_on_taps(rng, taps, fill):
    """W3[m][x][y] of zeros but for `taps` of the 25 taps; fill(rng) gives a tap's 32 channel weights."""
    w3 = np.zeros((32, 5, 5))
    for t in rng.choice(25, taps, replace=False):
        w3[:, t // 5, t % 5] = fill(rng)
    return w3


def _ints(top):
    return lambda rng, h, w: rng.integers(0, top + 1, (h, w)).astype(np.float32)


def weight_sets():
    """{name: (blob, plane(rng, h, w), X, budget)}: the weight blob, how the set draws its upscaled plane, the operands whose lo
    piece the set is about (condition (c)) and the set's budget for (sum|terms| + |C|) / q.

    All weights are small integers times a power of two, so every product is a multiple of its layer's q.  A layer's q is the
    product of its operands' last bits and is carried forward, while the sums grow against it: where the operands of one layer
    are wide, the layers behind it are sparse.  And a product of two twelve-bit operands alone is 2^22 q, so no single product
    has both operands wide: in wide-c1/W2 and wide-c2/W3 the wide activations meet narrow weights and the wide weights meet
    narrow (small integer) activations, channel by channel -- which is also what separates the two lo-piece terms wh xl and wl xh.
    Every set meets the budget 2^21 with the output resolved: b3 = 128 and the last fmaf is exact on every sample."""
    sets = {}

    # dense: every tap and channel non-zero; integer W1 in +-1..12, W2 in +-1..3, W3 in +-1..5 (x 2^-13, to leave the clamp), integer
    # Y in 0..3, negative integer biases.  The ranges hold 24, 6 and 10 values against 81 taps and 64 / 32 channels, so values
    # repeat; what the range allows is that any two taps or channels differ in most of the channels they feed.  All weights and Y
    # are narrow (lo = 0) and the activations are integers below 2^22, which hi + lo hold exactly: model == plain.
    rng = np.random.default_rng(SEED)
    sets["dense"] = (pack(-rng.integers(1, 9, 64), _signed(rng, 12, (64, 9, 9)), -rng.integers(1, 33, 32), _signed(rng, 3, (32, 64)),
                          128.0, _signed(rng, 5, (32, 5, 5)) * 2.0 ** -13), _ints(3), (), 2.0 ** 21)

    # wide-Y: Y = odd / 1024 in [2, 4): twelve significant bits, yl = +-2^-10 on every sample (a tie of the fp16 rounding each time:
    # round to nearest EVEN decides the sign).  W1 = +-1 on all 81 taps (the unsplit tap (8,8) included).  Layer 2 reads 3 channels
    # per output, layer 3 a channel of its own on each of the 25 taps.
    rng = np.random.default_rng(SEED + 1)
    sets["wide-Y"] = (pack(-rng.integers(1, 5, 64), _signed(rng, 1, (64, 9, 9)), -rng.integers(1, 5, 32),
                           _rows_of(rng, 32, 64, 3, _one_negative(2)), 128.0,
                           _w3_one_channel(rng, 25) * 2.0 ** -5),
                      lambda rng, h, w: ((2049 + 2 * rng.integers(0, 1024, (h, w))) / 1024.0).astype(np.float32), ("Y",), 2.0 ** 21)

    # wide-W1: three in ten of the W1 weights are +-(2048 + odd) / 256, lo piece +-1 / 256 (x 2^8: +-1); the others +-1..7; integer Y
    # in 0..3.  c1 has eight fractional bits behind it: layer 2 reads 4 channels per output, layer 3 a channel of its own on each
    # of 12 taps.
    rng = np.random.default_rng(SEED + 2)
    w1 = np.where(rng.random((64, 9, 9)) < 0.3, _wide(rng, (64, 9, 9)) / 256.0, _signed(rng, 7, (64, 9, 9)))
    sets["wide-W1"] = (pack(-rng.integers(1, 9, 64), w1, -rng.integers(1, 5, 32), _rows_of(rng, 32, 64, 4, _one_negative(2)),
                            128.0, _w3_one_channel(rng, 12) * 2.0 ** -6),
                       _ints(3), ("W1",), 2.0 ** 21)

    # wide-c1/W2: integer Y in 0..3.  Two of three layer-1 channels have W1 in +-1..63 and b1 = 5000: c1 is an integer around 5000,
    # wide on most samples, and meets W2 = +-1..3 / 256.  Every third channel passes one sample of Y on, less 1 (c1 in 0..2), and
    # meets W2 = +-(2048 + odd) / 256.  W2 is dense; layer 3 reads a channel of its own on each of the 25 taps.
    rng = np.random.default_rng(SEED + 3)
    small = np.arange(2, 64, 3)
    b1 = np.full(64, 5000.0)
    b1[small] = -1
    w2 = _signed(rng, 3, (32, 64)) / 256.0
    w2[:, small] = _wide(rng, (32, small.size)) / 256.0
    sets["wide-c1/W2"] = (pack(b1, _single_tap(rng, _signed(rng, 63, (64, 9, 9)), small), -rng.integers(1, 5, 32), w2, 128.0,
                               _w3_one_channel(rng, 25) * 2.0 ** -6),
                          _ints(3), ("c1", "W2"), 2.0 ** 21)

    # wide-c2/W3: integer Y in 0..3, W1 and c1 as in dense (W1 in +-1..7) but for channels 60..63, which pass one sample of Y on,
    # less 1.  Two of three layer-2 channels read channels 0..59 densely with W2 in +-1..3 and b2 = 5000: c2 is an integer around
    # 5000, wide on most samples, and meets W3 = +-1..2 / 2048.  Every third channel is one of channels 60..63 (c2 in 0..2) and
    # meets W3 = +-(2048 + odd) / 2048.  Layer 3 reads 2 channels of either kind on each of the 25 taps.
    rng = np.random.default_rng(SEED + 4)
    small = np.arange(2, 32, 3)
    big = np.setdiff1d(np.arange(32), small)
    b1 = -rng.integers(1, 9, 64).astype(np.float64)
    b1[60:] = -1
    w2 = _signed(rng, 3, (32, 64)).astype(np.float64)
    w2[:, 60:] = 0
    w2[small] = _rows_of(rng, small.size, 64, 1, lambda r, n: np.ones(n), among=np.arange(60, 64))
    b2 = np.full(32, 5000.0)
    b2[small] = 0

    def taps_w3(r):
        w = _rows_of(r, 1, 32, 2, lambda q, n: _signed(q, 2, n), among=big)[0]
        return w + _rows_of(r, 1, 32, 2, lambda q, n: _wide(q, n), among=small)[0]
    sets["wide-c2/W3"] = (pack(b1, _single_tap(rng, _signed(rng, 7, (64, 9, 9)), range(60, 64)), b2, w2, 128.0,
                               _w3_on_taps(rng, 25, taps_w3) / 2048.0), _ints(3), ("c2", "W3"), 2.0 ** 21)
    return sets


def cases():
    """[(name, blob, up, X, budget)]: dense at every shape, each wide set at WIDE_SHAPES, dense at BAND_SHAPE last."""
    out = []
    for i, (name, (blob, plane, x, budget)) in enumerate(weight_sets().items()):
        for h, w in (SHAPES + [BAND_SHAPE] if name == "dense" else WIDE_SHAPES):
            rng = np.random.default_rng(SEED + 100 * i + 7 * h + w)
            up = plane(rng, h, w)
            if not up.any():
                up = up + np.float32(1.0)        # (a 1 x 1 plane may draw 0, and every layer would then pass its bias on)
            up.setflags(write=False)
            out.append(("%s %dx%d" % (name, w, h), blob, up, x, budget))
    return out

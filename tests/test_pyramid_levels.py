"""k_pyramid_level and k_pyramid_fused (orb-slam-_amd/csrc/orbx_pyramid.hip) at every kernel form, level-0
alignment, width class and band edge, and the oracle's resize against two references of its own.

  np_resize       cv::resize INTER_LINEAR u8 restated in numpy integers from SURVEY.md A.2: per-axis tables
                  (tap 0, tap 1, a0, a1) from float32 coordinates, 11-bit coefficients rounded to nearest, the
                  scalar vertical pass (h0 b0 + h1 b1 + 2^21) >> 22 and the SSE2 one
                  ((((h0 >> 4) b0) >> 16) + (((h1 >> 4) b1) >> 16) + 2) >> 2 below the SIMD end.  The CPU tests hold
                  the oracle (oracle/orbref.c) to it byte for byte, and both to a float64 bilinear interpolation
                  within bounds that follow from the number formats alone.
  window          from the same tables, whether every 4-column group's eight taps lie within 8 bytes of its first
                  tap (LevelGeom::pyr_win, ensure_geometry): the CPU tests prove which scale factors of the GPU
                  cases take the byte-window path and which the per-byte one.
  GPU tests       one handle per case on a batch of distinct frames that cycles five image classes (uniform
                  noise, 0/255 noise, all-255, all-0, 1-px checkerboard); every level of every frame must equal
                  orbref.resize_linear chained from level 0, with the workspace filled with 0x00 and with 0xFF
                  before the run, and debug_launches proves the form (fused groups or one launch per level).

Not here on purpose: frames at the edge of an allocation (a staging read that left it would be a fault, not a
wrong byte; the sentinel layouts catch a skipped or an extra chunk as changed bytes), and timing.
"""
import os

import numpy as np
import pytest

SCALAR, SSE2 = 0, 1          # orbx.RESIZE_SCALAR / RESIZE_SSE2, orbref.RESIZE_*
MAX_BATCH_FUSED = 8          # kLatencyMaxBatch: batches up to this size take the fused groups
PYR_ROWS = 12                # kPyrRows: output rows per block of k_pyramid_level
BAND_ROWS = 4                # pyr_plan: rows of a group's last level per band


# ---------------------------------------------------------------------------------------------------------
# 1. the independent references
# ---------------------------------------------------------------------------------------------------------
def axis_table(sn, dn):
    """SURVEY.md A.2's table of one axis: (tap 0, tap 1, a0, a1) per destination index."""
    scale = float(sn) / float(dn)
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    fr = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= sn - 1
    s[lo], fr[lo] = 0, 0
    s[hi], fr[hi] = sn - 1, 0
    a0 = np.rint((np.float32(1) - fr) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fr * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, sn - 1), a0, a1


def simd_end(w):
    """Columns VResizeLinearVec_32s8u covers: 16 at a time while x <= w - 16, then 4 at a time while x < w - 4."""
    x = 0
    while x <= w - 16:
        x += 16
    while x < w - 4:
        x += 4
    return x


def np_resize(src, dw, dh, mode):
    sh, sw = src.shape
    x0, x1, a0, a1 = axis_table(sw, dw)
    y0, y1, b0, b1 = axis_table(sh, dh)
    S = src.astype(np.int64)
    H = S[:, x0] * a0 + S[:, x1] * a1
    h0, h1, b0, b1 = H[y0], H[y1], b0[:, None], b1[:, None]
    out = (h0 * b0 + h1 * b1 + (1 << 21)) >> 22
    if mode == SSE2:
        e = simd_end(dw)
        out[:, :e] = (((((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16) + 2) >> 2)[:, :e]
    return np.clip(out, 0, 255).astype(np.uint8)


def exact_bilinear(src, dw, dh):
    """Bilinear interpolation in float64 with the same half-pixel mapping and clamps, no quantisation."""
    def axis(sn, dn):
        f = (np.arange(dn, dtype=np.float64) + 0.5) * (float(sn) / float(dn)) - 0.5
        s = np.floor(f).astype(np.int64)
        fr = f - s
        lo, hi = s < 0, s >= sn - 1
        s[lo], fr[lo] = 0, 0.0
        s[hi], fr[hi] = sn - 1, 0.0
        return s, np.minimum(s + 1, sn - 1), fr
    sh, sw = src.shape
    x0, x1, fx = axis(sw, dw)
    y0, y1, fy = axis(sh, dh)
    S = src.astype(np.float64)
    H = S[:, x0] * (1.0 - fx) + S[:, x1] * fx
    return H[y0] * (1.0 - fy)[:, None] + H[y1] * fy[:, None]


def window_ok(sw, sh, dw, dh):
    """LevelGeom::pyr_win restated: every 4-column group's taps within 8 bytes of its first tap, and the x4
    vertical sum below 2^32."""
    x0, x1, a0, a1 = axis_table(sw, dw)
    _, _, b0, b1 = axis_table(sh, dh)
    for g0 in range(0, dw, 4):
        c = np.minimum(np.arange(g0, g0 + 4), dw - 1)
        if (x0[c] < x0[g0]).any() or (x1[c] - x0[g0] > 7).any():
            return False
    return 4 * 255 * int((a0 + a1).max()) * int((b0 + b1).max()) + (1 << 23) < (1 << 32)


# ---------------------------------------------------------------------------------------------------------
# 2. frames
# ---------------------------------------------------------------------------------------------------------
def make_frames(seed, batch, H, W):
    """`batch` distinct frames that cycle the five image classes: uniform noise, 0/255 noise, all-255, all-0, 1-px
    checkerboard.  From the second cycle on the constant frames carry one inverted row and column and the
    checkerboard the other phase, so no two frames of a batch are equal."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((batch, H, W), np.uint8)
    for f in range(batch):
        k, cyc = f % 5, f // 5
        if k == 0:
            out[f] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        elif k == 1:
            out[f] = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
        elif k in (2, 3):
            v = 255 if k == 2 else 0
            out[f] = v
            if cyc:
                out[f, (7 * cyc) % H, :] = 255 - v
                out[f, :, (11 * cyc) % W] = 255 - v
        else:
            out[f] = (((yy + xx + cyc) & 1) * 255).astype(np.uint8)
    assert len({out[f].tobytes() for f in range(batch)}) == batch
    return out


# ---------------------------------------------------------------------------------------------------------
# 3. cases
# ---------------------------------------------------------------------------------------------------------
NFEAT = 300


class Case:
    """One handle on one batch.  layout: None for a contiguous tensor, else (offset, excess, odd): the frames are
    a view into a sentinel-filled flat tensor from byte `offset`, rows W + excess bytes apart, the frame stride
    odd or pitch * H.  env0: ORBX_PYR_FUSED=0 while the handle first sees the size.  levelled: the LDS fallback, a
    small batch on per-level launches without the switch."""

    def __init__(self, name, W, H, scale, nl, batch, mode, layout=None, env0=False, levelled=False, seed=1):
        self.name, self.W, self.H, self.scale, self.nl, self.batch, self.mode = name, W, H, scale, nl, batch, mode
        self.layout, self.env0, self.levelled, self.seed = layout, env0, levelled, seed

    @property
    def fused(self):
        return self.batch <= MAX_BATCH_FUSED and not self.env0 and not self.levelled

    @property
    def launches(self):
        """debug_launches' pyramid count: the groups {1..3} and {4..} of the fused form, else one per level.
        (Two levels give 1 in either form; there the batch size alone decides, as launch_pyramid does.)"""
        if self.fused:
            return 1 if self.nl <= 4 else 2
        return self.nl - 1

    def __repr__(self):
        return self.name


# (offset, pitch excess, odd frame stride): every offset of {0, 1, 3, 4, 8, 15} and every excess of
# {0, 1, 2, 3, 4, 13, 16} once; (0, 2) and (8, 2) with pitch, base and frame stride all multiples of 4 on a 150-px
# row keep kA, the others lose it with a start shift that changes from row to row or frame to frame
LAYOUTS = [(0, 0, True), (1, 1, True), (3, 2, True), (4, 3, True), (8, 4, True), (15, 13, True), (4, 16, True),
           (0, 2, False), (8, 2, False)]
MODE_NAME = {SCALAR: "scalar", SSE2: "sse2"}


def _per_level_cases():
    B = MAX_BATCH_FUSED + 1
    out = []
    # level-1 widths 80..84: w mod 4 = 0, 1, 2, 3, 0 and an SSE2 scalar tail of 0, 1, 2, 3, 4 columns; level-1
    # heights mod 12 = 0, 1, 11 (and others); row blocks x 9 frames: 63 (h 84), 72 (h 85, 95)
    for W, H in [(96, 101), (97, 102), (98, 114), (100, 104), (101, 101)]:
        for mode in (SCALAR, SSE2):
            out.append(Case("w%d-%s" % (W, MODE_NAME[mode]), W, H, 1.2, 3, B, mode))
    # 154 -> 128 columns: rows without pitch padding
    out.append(Case("w154-nopad-scalar", 154, 112, 1.2, 3, B, SCALAR))
    out.append(Case("w154-nopad-sse2", 154, 112, 1.2, 3, B, SSE2))
    # q = ceil(w / 4) = 63, 64, 65 (level-1 widths 250, 256, 259): workgroups of 64, 64 and 128 threads
    for W, H, mode in [(300, 101, SCALAR), (307, 102, SSE2), (311, 114, SCALAR)]:
        out.append(Case("q%d-%s" % ((round(W / 1.2) + 3) // 4, MODE_NAME[mode]), W, H, 1.2, 3, B, mode))
    # q = 261 > 256: the second trip of the group loop
    out.append(Case("q261-scalar", 1250, 80, 1.2, 2, B, SCALAR))
    out.append(Case("q261-sse2", 1250, 80, 1.2, 2, B, SSE2))
    # scale factors on both sides of the window predicate (test_window_predicate_splits_the_scales)
    for scale, W, H, nl in SCALE_SHAPES:
        for mode in (SCALAR, SSE2):
            out.append(Case("s%.1f-%dx%d-%s" % (scale, W, H, MODE_NAME[mode]), W, H, scale, nl, B, mode))
    # level-0 layouts, window path and per-byte path
    for i, lay in enumerate(LAYOUTS):
        for mode in (SCALAR, SSE2):
            out.append(Case("lay%d+%d%s-%s" % (lay[0], lay[1], "odd" if lay[2] else "", MODE_NAME[mode]), 150, 131,
                            1.2, 3, B, mode, layout=lay))
    out.append(Case("lay3+13odd-s2.5-scalar", 317, 211, 2.5, 2, B, SCALAR, layout=(3, 13, True)))
    out.append(Case("lay15+1odd-s2.5-sse2", 317, 211, 2.5, 2, B, SSE2, layout=(15, 1, True)))
    out.append(Case("tall-scalar", 120, 180, 1.2, 3, B, SCALAR))
    out.append(Case("tall-sse2", 120, 180, 1.2, 3, B, SSE2))
    out.append(Case("wide-short-scalar", 600, 92, 1.2, 3, B, SCALAR))
    out.append(Case("wide-short-sse2", 600, 92, 1.2, 3, B, SSE2))
    return out


# (scale, W, H, levels): three levels where 62 px are left, so that level 2 runs from an always-aligned source
SCALE_SHAPES = [(1.1, 200, 160, 3), (1.2, 150, 131, 3), (1.6, 200, 160, 3), (2.0, 320, 200, 2), (2.0, 330, 250, 3),
                (2.2, 317, 211, 2), (2.5, 317, 211, 2), (3.0, 320, 200, 2)]
WINDOW_SCALES, BYTE_SCALES = (1.1, 1.2, 1.6), (2.2, 2.5, 3.0)   # 2.0: by size (320 -> 160 window, 165 -> 82 not)

# The LDS fallback: at scale 2.0 and four levels (500 -> 250 -> 125 -> 62 rows) a band of 4 level-3 rows needs up
# to 18 rows of level 1 and 36 of level 0, so the group's two LDS buffers take 36 (W + 30) + 18 (W / 2 + 15) + 16
# bytes, rounded up to 16-byte row pitches, and pass 160 KiB from about W = 3610 (3900: 176,272 bytes), while a
# per-level launch stages 12 x 2 + 2 = 26 rows (3900: 101,936 bytes; 160 KiB at about W = 6270).  3900 x 500 is on
# the fallback side, 3400 x 500 on the fused one; test_lds_fallback_threshold asserts both with debug_launches.
FALLBACK_SHAPE, FUSED_NEIGHBOUR = (3900, 500, 2.0, 4), (3400, 500, 2.0, 4)


def _fused_cases():
    out = []
    # level counts: one group of 1, 2 and 3 levels, the second group with one level and in full
    for nl, batch in [(2, 1), (3, 2), (4, 8), (5, 1), (8, 2), (8, 8)]:
        for mode in (SCALAR, SSE2):
            out.append(Case("n%d-b%d-%s" % (nl, batch, MODE_NAME[mode]), 301, 263, 1.2, nl, batch, mode))
    # the most levels 260 x 230 holds at scale 1.1 (level 13 is 75 x 67; a 15th would be 61 rows): the handle
    # itself takes up to kMaxLevels = 16
    out.append(Case("n14-s1.1-scalar", 260, 230, 1.1, 14, 2, SCALAR))
    out.append(Case("n14-s1.1-sse2", 260, 230, 1.1, 14, 1, SSE2))
    for i, lay in enumerate(LAYOUTS):
        for mode in (SCALAR, SSE2):
            out.append(Case("lay%d+%d%s-%s" % (lay[0], lay[1], "odd" if lay[2] else "", MODE_NAME[mode]), 150, 131,
                            1.2, 3, (1, 2, 8)[i % 3] if lay[2] else 2, mode, layout=lay))
    out.append(Case("lay3+13odd-s2.5-scalar", 317, 211, 2.5, 2, 2, SCALAR, layout=(3, 13, True)))
    out.append(Case("lay15+1odd-s2.5-sse2", 317, 211, 2.5, 2, 2, SSE2, layout=(15, 1, True)))
    # widest computed level 1042, 1833 and 2083 columns: 320 and 512 threads, and q = 521 > 512 wraps the items
    for W, batch, mode in [(1250, 2, SCALAR), (1250, 1, SSE2), (2200, 1, SCALAR), (2500, 1, SCALAR), (2500, 2, SSE2)]:
        out.append(Case("w%d-b%d-%s" % (W, batch, MODE_NAME[mode]), W, 80, 1.2, 2, batch, mode))
    out.append(Case("w1250-n3-scalar", 1250, 92, 1.2, 3, 1, SCALAR))   # three levels: the launch count tells the form
    # the group's last level 64, 65 and 67 rows: a full, a 1-row and a 3-row last band
    for H, mode in [(92, SCALAR), (94, SSE2), (96, SCALAR)]:
        out.append(Case("h%d-%s" % (H, MODE_NAME[mode]), 149, H, 1.2, 3, 2, mode))
    for scale, W, H, nl in SCALE_SHAPES:
        for mode in (SCALAR, SSE2):
            out.append(Case("s%.1f-%dx%d-%s" % (scale, W, H, MODE_NAME[mode]), W, H, scale, nl, 2, mode))
    out.append(Case("env0-lay1+1odd-scalar", 150, 131, 1.2, 3, 2, SCALAR, layout=(1, 1, True), env0=True))
    out.append(Case("env0-lay15+13odd-sse2", 150, 131, 1.2, 3, 8, SSE2, layout=(15, 13, True), env0=True))
    W, H, scale, nl = FALLBACK_SHAPE
    out.append(Case("lds-fallback", W, H, scale, nl, 1, SCALAR, levelled=True))
    return out


PER_LEVEL, FUSED = _per_level_cases(), _fused_cases()
HOST_SHAPES = [(150, 131, 1.2, 3, SCALAR), (301, 263, 1.2, 8, SSE2), (317, 211, 2.5, 2, SCALAR)]
REUSE_A, REUSE_B = (150, 131), (200, 160)


def all_shapes():
    s = {(c.W, c.H, c.scale, c.nl) for c in PER_LEVEL + FUSED}
    s |= {(W, H, scale, nl) for W, H, scale, nl, _ in HOST_SHAPES}
    s |= {(W, H, 1.2, 3) for W, H in (REUSE_A, REUSE_B)}
    s.add(FUSED_NEIGHBOUR)
    return sorted(s)


def sizes_of(orbref, W, H, scale, nl):
    return orbref.level_sizes(orbref.make_params(NFEAT, scale, nl, 20, 7), W, H)


def chain(orbref, frame, sizes, mode, resize=None):
    """ComputePyramid: every level from the one before."""
    resize = resize or orbref.resize_linear
    lv = [frame]
    for w, h in sizes[1:]:
        lv.append(resize(lv[-1], w, h, mode))
    return lv


_refs = {}


def reference(orbref, W, H, scale, nl, batch, mode, seed):
    """(frames, [frame][level] oracle bytes), computed once per key and shared; nobody writes to it."""
    key = (W, H, scale, nl, batch, mode, seed)
    if key not in _refs:
        frames = make_frames(seed, batch, H, W)
        sizes = sizes_of(orbref, W, H, scale, nl)
        levels = [chain(orbref, frames[f], sizes, mode) for f in range(batch)]
        frames.setflags(write=False)
        for lv in levels:
            for a in lv:
                a.setflags(write=False)
        _refs[key] = (frames, levels)
    return _refs[key]


# ---------------------------------------------------------------------------------------------------------
# 4. CPU: the oracle's resize against the restatement and the exact interpolation
# ---------------------------------------------------------------------------------------------------------
def test_simd_end_equals_oracle(orbref):
    for w in range(1, 301):
        assert simd_end(w) == orbref.resize_simd_end(w), w
    # the tails the SSE2 cases are picked for
    assert [w - simd_end(w) for w in (80, 81, 82, 83, 84)] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("shape", all_shapes(), ids=lambda s: "%dx%d-s%.1f-n%d" % s)
def test_restatement_equals_oracle(orbref, shape):
    """Every level of every GPU case, the five image classes, both modes: byte for byte."""
    W, H, scale, nl = shape
    sizes = sizes_of(orbref, W, H, scale, nl)
    frames = make_frames(7, 5, H, W)
    for mode in (SCALAR, SSE2):
        for f in range(5):
            a = chain(orbref, frames[f], sizes, mode)
            b = chain(orbref, frames[f], sizes, mode, resize=np_resize)
            for l in range(1, nl):
                bad = np.argwhere(a[l] != b[l])
                assert bad.size == 0, "mode %d class %d level %d differs at %s" % (mode, f, l, bad[:3])


# Source sides below 512 px, where the float32 coordinates' own rounding stays below 0.01, and 1241 x 80 above it,
# held to the same bounds; scale factors from 1.1 to 3.0.  The oracle alone stays at 0.61 (scalar) and 0.82 (SSE2).
BOUND_SIZES = [(100, 90), (131, 97), (320, 77), (120, 180), (511, 64), (1241, 80)]
BOUND_SCALES = [1.1, 1.2, 1.6, 2.0, 2.2, 3.0]


@pytest.mark.parametrize("size", BOUND_SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_within_quantisation_of_exact_bilinear(orbref, size):
    """Scalar mode: |oracle - exact| < 0.75 = 0.5 (final rounding) + 4 * 255 * 0.5 / 2048 (each of the four
    products carries a coefficient rounded by at most half of 1/2048).  SSE2 columns: the two truncated high
    multiplies lose up to (1 + 1/32) quarter-pixels each, 0.516 px together, before the same rounding:
    -1.27 < oracle - exact < 0.75."""
    W, H = size
    frames = make_frames(11, 5, H, W)[[0, 1, 2, 4]]   # uniform noise, 0/255 noise, all-255, checkerboard
    worst = [0.0, 0.0, 0.0, 0.0]   # |scalar|, SSE2 columns max and min, |SSE2 mode's scalar tail|
    for scale in BOUND_SCALES:
        dw, dh = int(round(W / scale)), int(round(H / scale))
        e = simd_end(dw)
        for img in frames:
            exact = exact_bilinear(img, dw, dh)
            d = orbref.resize_linear(img, dw, dh, SCALAR).astype(np.float64) - exact
            s = orbref.resize_linear(img, dw, dh, SSE2).astype(np.float64) - exact
            worst[0] = max(worst[0], float(np.abs(d).max()))
            if e:
                worst[1] = max(worst[1], float(s[:, :e].max()))
                worst[2] = min(worst[2], float(s[:, :e].min()))
            if e < dw:
                worst[3] = max(worst[3], float(np.abs(s[:, e:]).max()))
    print("%dx%d: scalar %.3f, SSE2 columns +%.3f / %.3f, tail %.3f" % (W, H, *worst))
    assert worst[0] < 0.75 and worst[3] < 0.75, worst
    assert -1.27 < worst[2] and worst[1] < 0.75, worst


@pytest.mark.parametrize("mode", [SCALAR, SSE2])
def test_constant_images_stay_constant(orbref, mode):
    """All-255 stays all-255 and all-0 all-0 at every shape: the case the window path's "no saturation"
    argument (4 * 255 * sum(a) * sum(b) + 2^23 < 2^32) rests on."""
    for W, H, scale, nl in all_shapes():
        sizes = sizes_of(orbref, W, H, scale, nl)
        for v in (255, 0):
            for l, a in enumerate(chain(orbref, np.full((H, W), v, np.uint8), sizes, mode)):
                assert (a == v).all(), (W, H, scale, l, v)


def test_window_predicate_splits_the_scales(orbref):
    """LevelGeom::pyr_win from the restated tables, per computed level of the scale cases: the byte window
    holds at 1.1, 1.2 and 1.6, fails at 2.2, 2.5 and 3.0, and at 2.0 holds where the source width is even all
    the way (320 -> 160) and fails where a level's ratio is just above 2 (165 -> 82).  Both paths of both
    kernels therefore run in the GPU cases."""
    win = {}
    for scale, W, H, nl in SCALE_SHAPES:
        sizes = sizes_of(orbref, W, H, scale, nl)
        win[(scale, W)] = [window_ok(*sizes[l - 1], *sizes[l]) for l in range(1, nl)]
    for (scale, W), v in win.items():
        if scale in WINDOW_SCALES:
            assert all(v), (scale, W, v)
        if scale in BYTE_SCALES:
            assert not any(v), (scale, W, v)
    assert win[(2.0, 320)] == [True] and win[(2.0, 330)] == [True, False]
    # the layout cases: 150 x 131 at 1.2 on the window, 317 x 211 at 2.5 on the bytes
    s = sizes_of(orbref, 150, 131, 1.2, 3)
    assert window_ok(*s[0], *s[1]) and window_ok(*s[1], *s[2])
    s = sizes_of(orbref, 317, 211, 2.5, 2)
    assert not window_ok(*s[0], *s[1])


def test_carried_rows_occur_and_first_rows_never_repeat(orbref):
    """The window path keeps a source row's horizontal sums when the next output row's first tap row is this
    row's second (lo(y + 1) == hi(y)).  From the row tables: that happens on most rows at 1.1 and 1.2, on some
    up to a ratio just under 2, and never at 2.0 and above, so the cases run the loop both with and without a
    carried row.  A ratio above 1 also moves lo by at least one row per output row: lo(y + 1) == lo(y) never
    holds, which is why remembering lo instead of hi (docs/EXPERIMENTS.md, the pyramid suite's mutations) only
    switches the carry off and changes no byte."""
    share = {}
    for W, H, scale, nl in all_shapes():
        sizes = sizes_of(orbref, W, H, scale, nl)
        for l in range(1, nl):
            lo, hi, _, _ = axis_table(sizes[l - 1][1], sizes[l][1])
            assert (np.diff(lo) >= 1).all(), (W, H, scale, l)
            share.setdefault(scale, []).append(float((lo[1:] == hi[:-1]).mean()))
    assert min(share[1.1]) > 0.8 and min(share[1.2]) > 0.7 and 0.2 < min(share[1.6]) < 0.6
    assert max(share[2.2] + share[2.5] + share[3.0]) == 0.0
    s = sizes_of(orbref, 320, 200, 2.0, 2)
    lo, hi, _, _ = axis_table(s[0][1], s[1][1])
    assert not (lo[1:] == hi[:-1]).any()


def test_case_shapes_are_accepted_and_cover_the_classes(orbref):
    """Every size passes ensure_geometry's conditions (a FAST cell grid: 62 px on both sides; a quadtree root:
    w - 32 >= (h - 32) / 2), and the per-level cases hit the classes they are named for."""
    for W, H, scale, nl in all_shapes():
        for w, h in sizes_of(orbref, W, H, scale, nl):
            assert w >= 62 and h >= 62 and (w - 32) >= 0.5 * (h - 32), (W, H, scale, nl, w, h)
    l1 = [sizes_of(orbref, c.W, c.H, c.scale, c.nl)[1] for c in PER_LEVEL]
    assert {w % 4 for w, _ in l1} == {0, 1, 2, 3} and any(w % 64 == 0 for w, _ in l1)
    assert {w - simd_end(w) for (w, _), c in zip(l1, PER_LEVEL) if c.mode == SSE2} >= {0, 1, 2, 3, 4}
    assert {h % PYR_ROWS for _, h in l1} >= {0, 1, 11}
    assert {(w + 3) // 4 for w, _ in l1} >= {63, 64, 65} and max((w + 3) // 4 for w, _ in l1) > 256
    blocks = {((h + PYR_ROWS - 1) // PYR_ROWS) * (MAX_BATCH_FUSED + 1) % 8 == 0 for _, h in l1}
    assert blocks == {True, False}
    last = [sizes_of(orbref, c.W, c.H, c.scale, c.nl)[min(c.nl - 1, 3)] for c in FUSED]
    assert {h % BAND_ROWS for _, h in last} >= {0, 1, 3}
    widest = [sizes_of(orbref, c.W, c.H, c.scale, c.nl)[1][0] for c in FUSED]
    assert any(1024 < w <= 1792 for w in widest) and any(1792 < w <= 2048 for w in widest) and max(widest) > 2048


# ---------------------------------------------------------------------------------------------------------
# 5. GPU: device bytes against the oracle's
# ---------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def _device_frames(frames, cuda, layout):
    """The frames on the device: contiguous, or (offset, excess, odd) a view into a sentinel-filled flat tensor
    (rows W + excess apart from byte `offset`, frame stride pitch * H, made odd by 1 or 2 bytes if `odd`).
    Returns (view, parent)."""
    import torch
    host = torch.from_numpy(np.array(frames))   # a writable copy: the shared reference stays read-only
    if layout is None:
        t = host.to(cuda)
        return t, None
    offset, excess, odd = layout
    B, H, W = frames.shape
    pitch = W + excess
    stride = pitch * H
    if odd:
        stride += 1 if stride % 2 == 0 else 2
    parent = torch.full((offset + B * stride + 64,), SENTINEL, dtype=torch.uint8, device=cuda)
    view = parent.as_strided((B, H, W), (stride, pitch, 1), offset)
    view.copy_(host.to(cuda))
    assert view.data_ptr() == parent.data_ptr() + offset and view.stride(1) == pitch and view.stride(0) == stride
    return view, parent


class _fused_switch:
    """ORBX_PYR_FUSED=0 while a handle first sees a size (pyr_plan reads it then), restored afterwards the way
    tests/test_gpu_parity.py test_pyramid_per_level_launches_small_batch does."""

    def __init__(self, off):
        self.off = off

    def __enter__(self):
        if self.off:
            os.environ["ORBX_PYR_FUSED"] = "0"
        else:
            os.environ.pop("ORBX_PYR_FUSED", None)

    def __exit__(self, *exc):
        os.environ.pop("ORBX_PYR_FUSED", None)


def _compare(got, want, tag):
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, "%s level %d: %s against %s" % (tag, l, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            assert False, "%s level %d: %d bytes differ, first (y, x) %s: device %s oracle %s" % (
                tag, l, len(bad), bad[:4].tolist(), a[tuple(bad[:4].T)].tolist(), b[tuple(bad[:4].T)].tolist())


def _run_device_case(orbref, cuda, c):
    import torch
    import orbx
    sizes = sizes_of(orbref, c.W, c.H, c.scale, c.nl)
    frames, want = reference(orbref, c.W, c.H, c.scale, c.nl, c.batch, c.mode, c.seed)
    ex = orbx.ORBextractor(NFEAT, c.scale, c.nl, 20, 7)
    ex.set_cv_modes(c.mode, 0)
    with _fused_switch(c.env0):
        got = ex.debug_launches(c.H, c.W, c.batch)
    assert got["pyramid"] == c.launches, (c.name, got)
    assert got["pyramid_sources"] == ((1 | (8 if c.nl > 4 else 0)) if c.fused else (1 << (c.nl - 1)) - 1), (c.name, got)
    imgs, parent = _device_frames(frames, cuda, c.layout)
    before = None if parent is None else parent.clone()
    cap = ex.capacity(c.H, c.W)
    kps = torch.zeros((c.batch, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.zeros((c.batch, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.zeros((c.batch,), dtype=torch.int32, device=cuda)
    s = torch.cuda.current_stream()
    # the first run sizes the workspace (a fill before it has nothing to fill) and makes these frames the
    # handle's last batch, which debug_pyramid reads; then the pyramid stage alone over 0x00 and the whole
    # extraction over 0xFF
    for fill in (None, 0x00, 0xFF):
        if fill is not None:
            ex.debug_fill_workspace(fill)
        if fill == 0x00:
            ex.extract_stage_device(0, imgs, kps, desc, counts)
        else:
            ex.extract_batch_device(imgs, kps, desc, counts)
        ex.sync(s)
        for f in range(c.batch):
            _compare(ex.debug_pyramid(f, sizes), want[f], "%s fill %s frame %d" % (c.name, fill, f))
    if parent is not None:
        assert torch.equal(parent, before), "%s: the caller's buffer changed" % c.name
    ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", PER_LEVEL, ids=repr)
def test_per_level_form(orbref, cuda, case):
    """k_pyramid_level: batch 9, one launch per level."""
    assert not case.fused and case.launches == case.nl - 1
    _run_device_case(orbref, cuda, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED, ids=repr)
def test_fused_form(orbref, cuda, case):
    """k_pyramid_fused: batches of 1, 2 and 8, one launch per level group; with ORBX_PYR_FUSED=0 and past the
    LDS limit the same batches on k_pyramid_level."""
    _run_device_case(orbref, cuda, case)


@pytest.mark.gpu
def test_lds_fallback_threshold(orbref, cuda):
    """FALLBACK_SHAPE's group outgrows 160 KiB of LDS and goes per level at batch 1; a narrower neighbour stays
    fused (its bytes: the lds-fallback case of test_fused_form)."""
    import orbx
    for (W, H, scale, nl), want in ((FALLBACK_SHAPE, nl_launches(FALLBACK_SHAPE[3], False)),
                                    (FUSED_NEIGHBOUR, nl_launches(FUSED_NEIGHBOUR[3], True))):
        ex = orbx.ORBextractor(NFEAT, scale, nl, 20, 7)
        assert ex.debug_launches(H, W, 1)["pyramid"] == want, (W, H)
        assert ex.debug_launches(H, W, MAX_BATCH_FUSED + 1)["pyramid"] == nl - 1
        ex.close()


def nl_launches(nl, fused):
    return (1 if nl <= 4 else 2) if fused else nl - 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "%dx%d-s%.1f-n%d-m%d" % s)
def test_host_call(orbref, cuda, shape):
    """ex(img) re-pitches the image (rows at align64(W), base aligned) and replays a graph: the fused form on an
    aligned level 0, read back through mvImagePyramid.  A strided numpy view goes the same way."""
    import orbx
    W, H, scale, nl, mode = shape
    frames, want = reference(orbref, W, H, scale, nl, 5, mode, 21)
    ex = orbx.ORBextractor(NFEAT, scale, nl, 20, 7)
    ex.set_cv_modes(mode, 0)
    assert ex.debug_launches(H, W, 1)["pyramid"] == nl_launches(nl, True)
    ex(frames[0])
    for fill in (0x00, 0xFF):
        for f in range(5):
            ex.debug_fill_workspace(fill)
            if f == 4:   # a view with a row step of W + 7
                wide = np.full((H, W + 7), SENTINEL, np.uint8)
                wide[:, 3:3 + W] = frames[f]
                ex(wide[:, 3:3 + W])
            else:
                ex(frames[f])
            _compare(ex.mvImagePyramid, want[f], "host fill %#x frame %d" % (fill, f))
    ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", 2, MAX_BATCH_FUSED + 1], ids=["host", "fused", "per-level"])
def test_handle_reuse(orbref, cuda, how):
    """Two batches of one shape back to back through one handle, another shape, then the first again: every
    result is that batch's own bytes (no stale cached level, table or plan)."""
    import torch
    import orbx
    nb = 1 if how == "host" else how
    ex = orbx.ORBextractor(NFEAT, 1.2, 3, 20, 7)
    s = torch.cuda.current_stream()
    for step, ((W, H), seed) in enumerate([(REUSE_A, 31), (REUSE_A, 32), (REUSE_B, 33), (REUSE_A, 31), (REUSE_B, 34)]):
        frames, want = reference(orbref, W, H, 1.2, 3, nb, SCALAR, seed)
        sizes = sizes_of(orbref, W, H, 1.2, 3)
        if how == "host":
            ex(frames[0])
            _compare(ex.mvImagePyramid, want[0], "reuse host step %d" % step)
            continue
        assert ex.debug_launches(H, W, nb)["pyramid"] == nl_launches(3, nb <= MAX_BATCH_FUSED)
        imgs, _ = _device_frames(frames, cuda, None if step % 2 else (1, 3, True))
        cap = ex.capacity(H, W)
        kps = torch.zeros((nb, cap, 7), dtype=torch.int32, device=cuda)
        desc = torch.zeros((nb, cap, 32), dtype=torch.uint8, device=cuda)
        counts = torch.zeros((nb,), dtype=torch.int32, device=cuda)
        ex.extract_batch_device(imgs, kps, desc, counts)
        ex.sync(s)
        for f in range(nb):
            _compare(ex.debug_pyramid(f, sizes), want[f], "reuse b%d step %d frame %d" % (nb, step, f))
    ex.close()

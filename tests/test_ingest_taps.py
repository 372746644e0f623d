"""Image ingest, both tap paths of csrc/orbx_ingest.hip at every alignment, border and channel order.

ig_remap_pixel has an interior fast path (0 <= sx < xlim, 0 <= sy < rows - 1: aligned 8/12-byte loads, alignbyte,
v_perm, v_dot4, (X + 512) >> 10) and a checked path (ig_taps: an aligned window with a funnel shift when the
window lies inside the row, byte loads with the border value 0 otherwise).  launch_ingest switches the fast path
off (xlim = 0) for a source whose base, pitch or frame stride is not 4-byte aligned or whose row is narrower
than the load window.

The tap atlas enumerates map coordinates instead of drawing them.  Every coordinate is s + f/32 (exact in
float32), so the test knows sx, sy, fx, fy without rounding anything:
  cross     every sx in [-3, cols+2] x every sy in [-3, rows+2] x (fx, fy) in {0, 1, 16, 31}^2
  sweep     all 32 x 32 fractions at one position of each border class (inside, 4 edges, 4 corners)
  ties      s + (2k+1)/64 (x32 lands on k + 1/2: ties to even, k = 31 carries, s = -1 rounds to -0)
  specials  NaN, +-inf, +-3e9, +-1e6, 32767.5, -32768.5 in x, in y and in both
laid out row-major into maps 50 wide (50 = 2 mod 4: float4 and scalar map loads, dword and byte stores) with a
NaN tail.  Four orderings of the list give the map pairs of a batch.

The grid runs that atlas over cols 1..17, rows 1, 2, 5, the five (channels, order) cases and nine source
layouts (tight, padded, base + 1..3, pitch + 1..3, frame stride + 2) built as as_strided views of one flat
buffer whose padding holds a sentinel, into a contiguous destination and into an offset, padded out= view.
classify() restates the kernel's predicates and the CPU tests assert, per configuration, that every class the
grid claims (fast, window, per-byte, the border classes, the byte phases, both sides of xlim) is non-empty
where the geometry allows it and empty where it does not.  Every comparison is exact.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from test_ingest import np_ingest, np_round_x86

CASES = [(1, False), (3, False), (3, True), (4, False), (4, True)]
CASE_IDS = ["gray", "bgr", "rgb", "bgra", "rgba"]
COLS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17)
ROWS = (1, 2, 5)
BATCH = 3
DW = 50                      # atlas map width, 2 mod 4
SRC_PAD, DST_PAD = 0xA5, 0x5A
F32 = np.float32


# ---------------------------------------------------------------------------- the atlas

def _exact(s, f):
    """(coordinate, integer part, fraction) of s + f/32."""
    return (F32(s) + F32(f) / F32(32), s, f)


def _tie(s, k):
    """s + (2k+1)/64: x32 is 32 s + k + 1/2, which cvRound takes to the even neighbour."""
    r = 32 * s + k
    r += r & 1
    return (F32(s) + F32(2 * k + 1) / F32(64), r >> 5, r & 31)


# cvRound(m * 32) of NaN and of anything outside int is INT_MIN: fraction 0, integer part saturated to SHRT_MIN
SPECIALS = [(F32(np.nan), -32768, 0), (F32(np.inf), -32768, 0), (F32(-np.inf), -32768, 0), (F32(3e9), -32768, 0),
            (F32(-3e9), -32768, 0), (F32(1e6), 32767, 0), (F32(-1e6), -32768, 0), (F32(32767.5), 32767, 16),
            (F32(-32768.5), -32768, 16)]
TIES = [_tie(s, k) for s in (1, 0, -1) for k in (0, 1, 15, 30, 31)]
F4 = (0, 1, 16, 31)


def sweep_positions(rows, cols):
    """One position of every border class the geometry has, plus a second all-inside one at the far corner."""
    pos = sorted({(sx, sy) for sx in (-1, 0, cols - 1) for sy in (-1, 0, rows - 1)})
    if cols >= 2 and rows >= 2 and (cols - 2, rows - 2) not in pos:
        pos.append((cols - 2, rows - 2))
    return pos


@functools.lru_cache(maxsize=None)
def atlas(rows, cols):
    ent = []                                                                       # (x, y), each (m, s, f)
    for sy in range(-3, rows + 3):
        for sx in range(-3, cols + 3):
            ent += [(_exact(sx, fx), _exact(sy, fy)) for fy in F4 for fx in F4]
    n_cross = len(ent)
    for sx, sy in sweep_positions(rows, cols):
        ent += [(_exact(sx, fx), _exact(sy, fy)) for fy in range(32) for fx in range(32)]
    n_sweep = len(ent) - n_cross
    zero = _exact(0, 0)
    for t in TIES + SPECIALS:
        ent += [(t, zero), (zero, t), (t, t)]
    a = SimpleNamespace(n=len(ent), n_cross=n_cross, n_sweep=n_sweep)
    a.mx = np.array([e[0][0] for e in ent], F32)
    a.my = np.array([e[1][0] for e in ent], F32)
    a.sx = np.array([e[0][1] for e in ent], np.int64)
    a.fx = np.array([e[0][2] for e in ent], np.int64)
    a.sy = np.array([e[1][1] for e in ent], np.int64)
    a.fy = np.array([e[1][2] for e in ent], np.int64)
    return a


@functools.lru_cache(maxsize=None)
def atlas_maps(rows, cols):
    """(map_x, map_y, entry) as (4, drows, DW): the list forward, reversed (NaN pad in front), rolled by 1 and
    by 2, so that every entry meets other lanes, load branches and store branches.  entry is the atlas index
    (-1 in the pad)."""
    a = atlas(rows, cols)
    dr = a.n // DW + 1                                                             # never without a NaN tail

    def lay(v, fill):
        m = np.full(dr * DW, fill, v.dtype)
        m[:a.n] = v
        return np.stack([m, m[::-1], np.roll(m, 1), np.roll(m, 2)]).reshape(4, dr, DW)

    return lay(a.mx, np.nan), lay(a.my, np.nan), lay(np.arange(a.n), -1)


def make_frames(rows, cols, ch):
    """Three frames with distinct content per channel: random 1..255 (src[0, 0] and its neighbours are non-zero,
    so a NaN rounded to coordinate 0 shows), a 0/255 checkerboard whose phase depends on the channel, random."""
    rng = np.random.default_rng(1000 * rows + 10 * cols + ch)
    y, x, c = np.mgrid[0:rows, 0:cols, 0:ch]
    f = np.stack([rng.integers(1, 256, (rows, cols, ch)), ((x + y + c + 1) & 1) * 255,
                  rng.integers(1, 256, (rows, cols, ch))]).astype(np.uint8)
    return f[..., 0] if ch == 1 else f


PAIRS = ((0, 0), (1, 1), (2, 0), (2, 2))       # (frame, map): f % 2 for two map pairs, f for four

_REFS = {}


def refs(orbref, rows, cols, ch, rgb):
    """Frames, maps and expected outputs of one geometry, computed once.  The oracle and the numpy restatement
    must agree on every one of them."""
    key = (rows, cols, ch, rgb)
    if key not in _REFS:
        mx, my, ent = atlas_maps(rows, cols)
        frames = make_frames(rows, cols, ch)
        want = {}
        for f, m in PAIRS:
            want[f, m] = orbref.ingest(frames[f], rgb, mx[m], my[m])
            assert np.array_equal(want[f, m], np_ingest(frames[f], rgb, mx[m], my[m])), (key, f, m)
        plain = np.stack([orbref.ingest(frames[f], rgb) for f in range(BATCH)])
        for f in range(BATCH):
            assert np.array_equal(plain[f], np_ingest(frames[f], rgb)), (key, f)
        _REFS[key] = SimpleNamespace(mx=mx, my=my, ent=ent, frames=frames, plain=plain,
                                     want2=np.stack([want[f, f % 2] for f in range(BATCH)]),
                                     want4=np.stack([want[f, f] for f in range(BATCH)]))
    return _REFS[key]


# ---------------------------------------------------------------------------- layouts and the kernel's predicates

def layouts(rows, cols, ch):
    """(name, base, pitch, frame stride) in bytes."""
    rb = cols * ch
    p4 = (rb + 3) // 4 * 4 + 4
    up4 = lambda v: (v + 3) // 4 * 4
    out = [("tight", 0, rb, rows * rb), ("padded", 0, p4, rows * p4 + 8)]
    out += [("base+%d" % b, b, p4, rows * p4 + 8) for b in (1, 2, 3)]
    out += [("pitch+%d" % d, 0, p4 + d, up4(rows * (p4 + d)) + 4) for d in (1, 2, 3)]
    out += [("fstride+2", 0, p4, rows * p4 + 2)]
    return out


def xlim_of(cols, ch, base, pitch, fstride):
    """launch_ingest: fast iff 0 <= sx < xlim."""
    kw = 8 if ch == 1 else 12
    if (base | pitch | fstride) & 3 or cols * ch < kw:
        return 0
    return max(min(cols - 2, (cols * ch - kw) // ch) + 1, 0)


XS = ("left", "in", "right", "out")


def axis_state(s, n):
    """Per entry: which of the taps s, s + 1 lie in [0, n): 0 only the second (left / top border), 1 both,
    2 only the first (right / bottom border), 3 neither."""
    i0, i1 = (s >= 0) & (s < n), (s + 1 >= 0) & (s + 1 < n)
    return np.where(i0 & i1, 1, np.where(i1, 0, np.where(i0, 2, 3)))


def classify(a, rows, cols, ch, base, pitch, fstride, batch=BATCH):
    """Which path of ig_remap_pixel / ig_taps each atlas entry takes on this layout (base is the byte offset of
    the first pixel from a 4-byte aligned address)."""
    xlim = xlim_of(cols, ch, base, pitch, fstride)
    sx, sy = a.sx, a.sy
    fast = (sx >= 0) & (sx < xlim) & (sy >= 0) & (sy < rows - 1)
    kwb = 8 if ch == 1 else 12                                                     # 4 * kWords of ig_taps
    r = SimpleNamespace(xlim=xlim, fast=int(fast.sum()), window=0, bytes=0, fast_sh=set(), window_sh=set())
    for f in range(batch):
        r.fast_sh |= set(((base + f * fstride + sy[fast] * pitch + sx[fast] * ch) & 3).tolist())
        for yy in (sy, sy + 1):
            rowin = ~fast & (yy >= 0) & (yy < rows)
            row = base + f * fstride + np.clip(yy, 0, rows - 1) * pitch
            adr = row + sx * ch
            a4 = adr & ~3
            win = rowin & (sx >= 0) & (sx + 1 < cols) & (a4 >= row) & (a4 + kwb <= row + cols * ch)
            r.window += int(win.sum())
            r.bytes += int((rowin & ~win).sum())
            r.window_sh |= set((adr[win] & 3).tolist())
    r.fast_lo = bool((fast & (sx == xlim - 1)).any())                              # both sides of xlim, on fast rows
    r.fast_hi = bool(((sx == xlim) & (sy >= 0) & (sy < rows - 1)).any())
    return r


def window_possible(rows, cols, ch, base, pitch, fstride, batch=BATCH):
    """Some row holds an aligned 8/12-byte window: the first aligned address of the row plus the window fits.
    (Every aligned dword of a row holds the first byte of a pixel whose neighbour ends inside the window, and
    rows 0 and rows - 1 reach the checked path through sy = -1 and sy = rows - 1 on every layout.)"""
    kwb = 8 if ch == 1 else 12
    return any((-(base + f * fstride + y * pitch)) % 4 + kwb <= cols * ch for f in range(batch) for y in range(rows))


def border_counts(a, rows, cols):
    xs, ys = axis_state(a.sx, cols), axis_state(a.sy, rows)
    return {(XS[i], XS[j]): int(((xs == i) & (ys == j)).sum()) for i in range(4) for j in range(4)}


def border_possible(rows, cols):
    px = {"left": True, "in": cols >= 2, "right": True, "out": True}               # cols = 1: sx = 0 is "right"
    py = {"left": True, "in": rows >= 2, "right": True, "out": True}
    return {(i, j): px[i] and py[j] for i in XS for j in XS}


# ---------------------------------------------------------------------------- CPU: the atlas and its coverage

@pytest.mark.parametrize("rows", ROWS)
def test_atlas_is_what_it_says(rows):
    """The integer parts and fractions the atlas was built from are the ones cvRound(m * 32) gives, the maps
    hold every entry once per ordering, and every border class of the geometry is present."""
    for cols in COLS:
        a = atlas(rows, cols)
        for m, s, f in ((a.mx, a.sx, a.fx), (a.my, a.sy, a.fy)):
            r = np_round_x86(m * F32(32))
            assert np.array_equal(np.clip(r >> 5, -32768, 32767), s) and np.array_equal(r & 31, f)
        assert a.n_cross == (cols + 6) * (rows + 6) * 16 and a.n_sweep == 1024 * len(sweep_positions(rows, cols))
        mx, my, ent = atlas_maps(rows, cols)
        assert mx.shape[2] == DW and DW % 4 == 2 and mx.shape[1] >= 4              # rows of both alignments
        for k in range(4):
            assert np.array_equal(np.sort(ent[k][ent[k] >= 0]), np.arange(a.n))
            ok = ent[k] >= 0
            assert np.array_equal(mx[k][ok].view(np.int32), a.mx[ent[k][ok]].view(np.int32))
            assert np.array_equal(my[k][ok].view(np.int32), a.my[ent[k][ok]].view(np.int32))
            assert np.isnan(mx[k][~ok]).all() and np.isnan(my[k][~ok]).all() and (~ok).any()
        got, may = border_counts(a, rows, cols), border_possible(rows, cols)
        for cls in may:
            assert (got[cls] > 0) == may[cls], (rows, cols, cls, got[cls])
        # every sweep position carries all 1024 fractions
        sw = slice(a.n_cross, a.n_cross + a.n_sweep)
        for p, (sx, sy) in enumerate(sweep_positions(rows, cols)):
            q = slice(sw.start + 1024 * p, sw.start + 1024 * (p + 1))
            assert (a.sx[q] == sx).all() and (a.sy[q] == sy).all()
            assert len(set(zip(a.fx[q].tolist(), a.fy[q].tolist()))) == 1024
        # ties: the carry into the next integer, and the small negative that rounds to -0
        tie = {(float(m), int(s), int(f)) for m, s, f in zip(a.mx, a.sx, a.fx)}
        assert (1 + 63 / 64, 2, 0) in tie and (-1 / 64, 0, 0) in tie and (1 + 1 / 64, 1, 0) in tie
        assert (1 + 3 / 64, 1, 2) in tie and (-1 + 1 / 64, -1, 0) in tie


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_coverage_of_every_configuration(ch):
    """Per geometry and layout: each path the grid claims to run is reached by some atlas entry, and a path the
    geometry rules out is reached by none."""
    seen_fast_sh, seen_win_sh, n_fast_cfg = set(), set(), 0
    for rows in ROWS:
        for cols in COLS:
            a = atlas(rows, cols)
            assert len(layouts(rows, cols, ch)) == 9
            for name, base, pitch, fs in layouts(rows, cols, ch):
                cfg = (rows, cols, ch, name)
                assert pitch >= cols * ch and fs >= rows * pitch
                r = classify(a, rows, cols, ch, base, pitch, fs)
                aligned = not ((base | pitch | fs) & 3)
                assert aligned == (name == "padded" or (name == "tight" and cols * ch % 4 == 0)), cfg
                fast_possible = aligned and rows >= 2 and cols * ch >= (8 if ch == 1 else 12)
                assert (r.xlim > 0) == (aligned and cols * ch >= (8 if ch == 1 else 12)), cfg
                assert (r.fast > 0) == fast_possible, cfg
                assert (r.window > 0) == window_possible(rows, cols, ch, base, pitch, fs), cfg
                assert r.bytes > 0, cfg
                if fast_possible:
                    n_fast_cfg += 1
                    assert r.fast_lo and r.fast_hi, cfg                            # sx = xlim - 1 fast, xlim checked
                    assert r.fast_sh == {(s * ch) & 3 for s in range(r.xlim)}, cfg
                    if (ch == 1 and cols >= 11) or (ch == 3 and cols >= 7):
                        assert r.fast_sh == {0, 1, 2, 3}, cfg
                    seen_fast_sh |= r.fast_sh
                else:
                    assert not r.fast_sh, cfg
                if not aligned and cols * ch >= (8 if ch == 1 else 12) + 3:
                    assert r.window > 0, cfg                                       # the window off an unaligned base
                seen_win_sh |= r.window_sh
    assert n_fast_cfg > 0
    assert seen_fast_sh == ({0} if ch == 4 else {0, 1, 2, 3})
    assert seen_win_sh == {0, 1, 2, 3}


def test_xlim_restatement():
    assert xlim_of(16, 1, 0, 16, 64) == 9 and xlim_of(8, 1, 0, 8, 8) == 1 and xlim_of(7, 1, 0, 8, 8) == 0
    assert xlim_of(4, 3, 0, 12, 12) == 1 and xlim_of(5, 3, 0, 16, 16) == 2 and xlim_of(3, 3, 0, 12, 12) == 0
    assert xlim_of(3, 4, 0, 12, 12) == 1 and xlim_of(17, 4, 0, 68, 68) == 15 and xlim_of(2, 4, 0, 8, 8) == 0
    assert xlim_of(16, 1, 1, 16, 64) == 0 and xlim_of(16, 1, 0, 18, 64) == 0 and xlim_of(16, 1, 0, 16, 66) == 0


@pytest.mark.parametrize("ch,rgb", CASES, ids=CASE_IDS)
def test_oracle_matches_restatement_on_atlas(orbref, ch, rgb):
    """orbref.ingest == np_ingest on every atlas, every map ordering and the no-map path (asserted in refs())."""
    for rows in ROWS:
        for cols in COLS:
            g = refs(orbref, rows, cols, ch, rgb)
            assert g.want2.shape == (BATCH,) + g.mx.shape[1:] and g.plain.shape == (BATCH, rows, cols)
    g = refs(orbref, 5, 17, ch, rgb)
    assert g.want2.any() and not np.array_equal(g.want2[0], g.want2[2]) and not np.array_equal(g.want4[2], g.want2[2])


# ---------------------------------------------------------------------------- closed-form known answers

def closed_form_case(ch, v, alpha=77, rows=4, cols=12):
    """A constant image (v, v, v[, alpha]): every tap inside is v and every tap outside 0, so a pixel is
    (v wx wy 32 + 2^14) >> 15 with wx the summed weight of the x taps inside (fx, 32 or 32 - fx), wy likewise;
    all inside that is v; gray of (c, c, c) is c whatever alpha is.  Returns (src, map_x, map_y, want)."""
    src = np.full((rows, cols, ch), v, np.uint8)
    if ch == 4:
        src[..., 3] = alpha
    if ch == 1:
        src = src[..., 0]
    fy, fx = (t.reshape(-1) for t in np.mgrid[0:32, 0:32])
    mxs, mys, want = [], [], []
    for sx, wx in ((-1, fx), (1, 32 + 0 * fx), (cols - 1, 32 - fx)):
        for sy, wy in ((-1, fy), (1, 32 + 0 * fy), (rows - 1, 32 - fy)):
            mxs.append(F32(sx) + fx.astype(F32) / F32(32))
            mys.append(F32(sy) + fy.astype(F32) / F32(32))
            want.append((v * wx * wy * 32 + (1 << 14)) >> 15)
    shape = (9 * 32, 32)
    return (src, np.concatenate(mxs).reshape(shape), np.concatenate(mys).reshape(shape),
            np.concatenate(want).reshape(shape).astype(np.uint8))


CLOSED = [(ch, v) for ch in (1, 3, 4) for v in (1, 128, 255)]


@pytest.mark.parametrize("ch,v", CLOSED)
def test_closed_form(orbref, ch, v):
    src, mx, my, want = closed_form_case(ch, v)
    assert (want[4 * 32:5 * 32] == v).all()                                        # block 4: all inside, 1024 fractions
    fy = np.arange(32)[:, None]                                                    # block 5: the lower tap row outside
    assert np.array_equal(want[5 * 32:6 * 32], np.broadcast_to((v * (32 - fy) * 1024 + (1 << 14)) >> 15, (32, 32)))
    assert np.array_equal(want[3 * 32:4 * 32], np.broadcast_to((v * fy * 1024 + (1 << 14)) >> 15, (32, 32)))
    for rgb in (False, True):
        assert np.array_equal(orbref.ingest(src, rgb, mx, my), want)
        assert np.array_equal(np_ingest(src, rgb, mx, my), want)
        assert (orbref.ingest(src, rgb) == v).all() and (np_ingest(src, rgb) == v).all()


# ---------------------------------------------------------------------------- GPU: the grid

def device_src(frames, rows, cols, ch, lay, cuda):
    """The frames in one flat sentinel-filled device buffer, viewed through (base, pitch, frame stride)."""
    import torch
    _, base, pitch, fs = lay
    total = base + (BATCH - 1) * fs + (rows - 1) * pitch + cols * ch + 16
    flat = np.full(total, SRC_PAD, np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[base:], (BATCH, rows, cols, ch), (fs, pitch, ch, 1))
    view[...] = frames.reshape(BATCH, rows, cols, ch)
    dev = torch.from_numpy(flat).to(cuda)
    assert dev.data_ptr() % 4 == 0
    if ch == 1:
        return torch.as_strided(dev, (BATCH, rows, cols), (fs, pitch, 1), base)
    return torch.as_strided(dev, (BATCH, rows, cols, ch), (fs, pitch, ch, 1), base)


class OutView:
    """A destination view with base offset 1 and a padded pitch in a sentinel-filled flat buffer, and the
    bytes the whole buffer must hold after the call."""

    def __init__(self, want, cuda):
        import torch
        b, r, c = want.shape
        self.shape, self.strides = (b, r, c), (r * (c + 7) + 5, c + 7, 1)
        self.total = 1 + (b - 1) * self.strides[0] + (r - 1) * self.strides[1] + c + 9
        exp = np.full(self.total, DST_PAD, np.uint8)
        np.lib.stride_tricks.as_strided(exp[1:], self.shape, self.strides)[...] = want
        self.expect = torch.from_numpy(exp).to(cuda)
        self.cuda = cuda

    def fresh(self):
        import torch
        flat = torch.full((self.total,), DST_PAD, dtype=torch.uint8, device=self.cuda)
        return flat, torch.as_strided(flat, self.shape, self.strides, 1)


def same(got, want, what, entry=None):
    """Exact equality on the device; on a mismatch name the first bytes (and, through entry(index), the atlas
    entries they belong to)."""
    import torch
    if got.shape == want.shape and torch.equal(got, want):
        return
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = [tuple(int(v) for v in i) for i in np.argwhere(g != w)]
    first = [(i, int(g[i]), int(w[i])) + ((entry(i),) if entry else ()) for i in bad[:6]]
    pytest.fail("%s: %d of %d bytes differ; (index, got, want%s): %s"
                % (what, len(bad), g.size, ", entry" if entry else "", first))


def entry_of(a, ent, nmaps):
    """index (frame, y, x) of a remapped output -> the atlas entry behind it, as text."""
    def f(i):
        e = int(ent[i[0] % nmaps, i[1], i[2]])
        return "pad" if e < 0 else "sx %d fx %d sy %d fy %d (map %r, %r)" % (a.sx[e], a.fx[e], a.sy[e], a.fy[e],
                                                                             float(a.mx[e]), float(a.my[e]))
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rgb", CASES, ids=CASE_IDS)
def test_gpu_tap_grid(orbref, cuda, ch, rgb):
    """Every geometry x layout: three frames through two map pairs and through no map, into a contiguous
    destination and into an offset, padded out= view whose padding must keep its sentinel; four map pairs
    (more than frames) once per geometry.  Bit-exact against the oracle (== np_ingest, see refs())."""
    import torch
    import orbx
    for rows in ROWS:
        for cols in COLS:
            g, a = refs(orbref, rows, cols, ch, rgb), atlas(rows, cols)
            mx, my = torch.from_numpy(g.mx).to(cuda), torch.from_numpy(g.my).to(cuda)
            want2, want4 = torch.from_numpy(g.want2).to(cuda), torch.from_numpy(g.want4).to(cuda)
            plain = torch.from_numpy(g.plain).to(cuda)
            ov_map, ov_plain = OutView(g.want2, cuda), OutView(g.plain, cuda)
            for lay in layouts(rows, cols, ch):
                what = "rows %d cols %d ch %d rgb %d layout %s" % (rows, cols, ch, rgb, lay[0])
                src = device_src(g.frames, rows, cols, ch, lay, cuda)
                same(orbx.ingest_batch_device(src, rgb, mx[:2], my[:2]), want2, what + ", maps", entry_of(a, g.ent, 2))
                flat, view = ov_map.fresh()
                assert orbx.ingest_batch_device(src, rgb, mx[:2], my[:2], out=view) is view
                same(flat, ov_map.expect, what + ", maps, out= view (flat buffer)")
                same(orbx.ingest_batch_device(src, rgb), plain, what + ", no map")
                flat, view = ov_plain.fresh()
                orbx.ingest_batch_device(src, rgb, out=view)
                same(flat, ov_plain.expect, what + ", no map, out= view (flat buffer)")
                if lay[0] in ("tight", "padded", "base+1"):
                    same(orbx.ingest_batch_device(src, rgb, mx, my), want4, what + ", four map pairs",
                         entry_of(a, g.ent, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("ch,v", CLOSED)
def test_gpu_closed_form(cuda, ch, v):
    """The constant-image known answers through both tap paths: rows 4, cols 12 tight (aligned, so the inside
    block runs the fast path) and the same bytes one byte further on (every pixel on the checked path)."""
    import torch
    import orbx
    src, mx, my, want = closed_form_case(ch, v)
    dmx, dmy = torch.from_numpy(mx[None]).to(cuda), torch.from_numpy(my[None]).to(cuda)
    want = torch.from_numpy(want[None]).to(cuda)
    tight = torch.from_numpy(src[None]).to(cuda)
    flat = torch.full((tight.numel() + 1,), 200, dtype=torch.uint8, device=cuda)
    flat[1:] = tight.reshape(-1)
    for name, s in (("tight", tight), ("base+1", torch.as_strided(flat, tight.shape, tight.stride(), 1))):
        for rgb in (False, True):
            same(orbx.ingest_batch_device(s, rgb, dmx, dmy), want, "ch %d v %d %s rgb %d" % (ch, v, name, rgb))
            assert bool((orbx.ingest_batch_device(s, rgb) == v).all())


# ---------------------------------------------------------------------------- GPU: depth

DEPTH_F32 = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.17549435e-38, -1.17549435e-38, 2.3509887e-38,
                      np.inf, -np.inf, np.nan, 1.0, -1.0, 5000.0, 65535.0, 3.4028235e38, -3.4028235e38, 1e-20],
                     np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [0.5, 1.0 / 5000.0, 3.0])
def test_gpu_depth_f32(orbref, cuda, factor):
    """depth_type 1 with factor != 1, bit patterns: -0.0, denormals (in and out), inf and NaN."""
    import torch
    import orbx
    rng = np.random.default_rng(5)
    d = rng.uniform(0, 10, (2, 3, 37)).astype(np.float32)
    d[0, 0, :len(DEPTH_F32)] = DEPTH_F32
    d[1, 2, -len(DEPTH_F32):] = DEPTH_F32[::-1]
    out = orbx.depth_batch_device(torch.from_numpy(d).to(cuda), factor).cpu().numpy()
    for b in range(2):
        assert np.array_equal(bits(out[b]), bits(orbref.depth_convert(d[b], factor)))
    neg0 = bits(d) == np.int32(-2 ** 31)
    assert neg0.sum() == 2 and (bits(out)[neg0] == 0).all()                         # -0.0 * factor + 0.0f = +0.0
    assert np.isnan(out[0, 0, 11]) and out[0, 0, 9] == np.inf


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 3, 64, 65])
def test_gpu_depth_u16(orbref, cuda, cols):
    import torch
    import orbx
    d = np.random.default_rng(cols).integers(0, 65536, (2, 3, cols), dtype=np.uint16)
    d[0, 0, 0], d[1, 2, cols - 1], d[1, 0, 0] = 0, 65535, 65535
    d[0, 1, 0] = 0
    f = 1.0 / 5000.0
    out = orbx.depth_batch_device(torch.from_numpy(d.view(np.int16)).to(cuda), f).cpu().numpy()
    for b in range(2):
        assert np.array_equal(bits(out[b]), bits(orbref.depth_convert(d[b], f)))
    assert out[1, 0, 0] == np.float32(65535.0) * np.float32(f) and bits(out)[0, 0, 0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("isf", [False, True], ids=["u16", "f32"])
def test_gpu_depth_pitched(orbref, cuda, isf):
    """Source and destination as offset, padded views (whole elements) of sentinel-filled buffers, batch 3."""
    import torch
    import orbx
    b, rows, cols = 3, 4, 13
    rng = np.random.default_rng(9)
    if isf:
        d = rng.uniform(-5, 5, (b, rows, cols)).astype(np.float32)
        d[0, 0, :3], d[2, 3, -1] = (-0.0, 1e-40, np.inf), -0.0
        sflat = torch.full((3 + b * (rows * (cols + 5) + 1),), 777.0, dtype=torch.float32, device=cuda)
        payload = torch.from_numpy(d)
    else:
        d = rng.integers(0, 65536, (b, rows, cols), dtype=np.uint16)
        d[0, 0, 0], d[2, 3, -1] = 65535, 0
        sflat = torch.full((3 + b * (rows * (cols + 5) + 1),), 0x5A5A, dtype=torch.int16, device=cuda)
        payload = torch.from_numpy(d.view(np.int16))
    src = torch.as_strided(sflat, (b, rows, cols), (rows * (cols + 5) + 1, cols + 5, 1), 3)
    src.copy_(payload.to(cuda))
    dstr = (rows * (cols + 3) + 2, cols + 3, 1)
    total = 1 + b * dstr[0]
    f = 0.25
    exp = np.full(total, -123.0, np.float32)
    want = np.stack([orbref.depth_convert(d[i], f) for i in range(b)])
    np.lib.stride_tricks.as_strided(exp[1:], (b, rows, cols), tuple(4 * s for s in dstr))[...] = want
    dflat = torch.full((total,), -123.0, dtype=torch.float32, device=cuda)
    view = torch.as_strided(dflat, (b, rows, cols), dstr, 1)
    assert orbx.depth_batch_device(src, f, out=view) is view
    assert np.array_equal(bits(dflat.cpu().numpy()), bits(exp))
    assert np.array_equal(bits(orbx.depth_batch_device(src, f).cpu().numpy()), bits(want))


@pytest.mark.gpu
def test_gpu_depth_f32_unit_factor_is_identity(cuda):
    import torch
    import orbx
    t = torch.from_numpy(np.tile(DEPTH_F32, (1, 2, 1))).to(cuda)
    assert orbx.depth_batch_device(t, 1.0) is t
    assert orbx.depth_batch_device(t, 1.0 + 5e-6) is t                             # the reference's 1e-5 window


# ---------------------------------------------------------------------------- the argument contract

def raw_ingest(lib, src=0x1000, batch=1, rows=4, cols=8, ch=1, rgb=0, sstep=None, sfs=None, mx=None, my=None,
               nmaps=0, drows=None, dcols=None, dst=0x2000, dstep=None, dfs=None):
    """orbx_ingest_batch_device with valid defaults around the one argument under test.  Only for calls that
    return before a launch: the default pointers are not memory."""
    drows, dcols = rows if drows is None else drows, cols if dcols is None else dcols
    sstep = cols * ch if sstep is None else sstep
    dstep = dcols if dstep is None else dstep
    sfs = sstep * rows if sfs is None else sfs
    dfs = dstep * drows if dfs is None else dfs
    p = lambda v: C.c_void_p(v) if v else None
    return lib.orbx_ingest_batch_device(p(src), batch, rows, cols, ch, rgb, sstep, sfs, p(mx), p(my), nmaps, drows,
                                        dcols, p(dst), dstep, dfs, None)


REJECTED = {
    "channels 2": dict(ch=2),
    "channels 0": dict(ch=0),
    "channels 5": dict(ch=5),
    "src_step < cols * channels": dict(ch=3, sstep=23),
    "dst_step < dst_cols": dict(dstep=7),
    "dst_step < dst_cols (maps)": dict(mx=0x3000, my=0x4000, nmaps=1, drows=2, dcols=6, dstep=5),
    "map_x without map_y": dict(mx=0x3000, nmaps=1),
    "map_y without map_x": dict(my=0x4000, nmaps=1),
    "nmaps 0 with maps": dict(mx=0x3000, my=0x4000, nmaps=0),
    "nmaps -1 with maps": dict(mx=0x3000, my=0x4000, nmaps=-1),
    "no maps, dst rows differ": dict(drows=5),
    "no maps, dst cols differ": dict(dcols=7),
    "rows 32768": dict(rows=32768),
    "cols 32768": dict(cols=32768),
    "batch 2, src frame stride short": dict(batch=2, sfs=31),
    "batch 2, dst frame stride short": dict(batch=2, dfs=31),
    "batch -1": dict(batch=-1),
    "src NULL": dict(src=0),
    "dst NULL": dict(dst=0),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_ingest_rejects(name):
    """Each of these returns ORBX_EINVAL before any launch (no device needed)."""
    import orbx
    assert raw_ingest(orbx.lib, **REJECTED[name]) == orbx.EINVAL


def test_ingest_batch_zero_is_ok():
    import orbx
    assert raw_ingest(orbx.lib, batch=0) == orbx.OK
    assert raw_ingest(orbx.lib, batch=0, mx=0x3000, my=0x4000, nmaps=1, drows=3, dcols=5) == orbx.OK
    assert raw_ingest(orbx.lib, batch=0, ch=2) == orbx.EINVAL                        # still validated


@pytest.mark.gpu
def test_gpu_ingest_contract_through_wrapper(cuda):
    """The wrapper raises OrbxError(EINVAL) and leaves the destination alone; batch 0 writes nothing."""
    import torch
    import orbx
    src = torch.full((2, 4, 8, 3), 9, dtype=torch.uint8, device=cuda)
    maps = torch.zeros((1, 4, 8), dtype=torch.float32, device=cuda)
    out = torch.full((2, 4, 8), DST_PAD, dtype=torch.uint8, device=cuda)
    bad = [lambda: orbx.ingest_batch_device(src[..., :2], out=out),                                   # channels 2
           lambda: orbx.ingest_batch_device(torch.as_strided(src, (2, 4, 8, 3), (96, 23, 3, 1)), out=out),
           lambda: orbx.ingest_batch_device(src, False, maps, maps, out=torch.as_strided(out, (2, 4, 8), (32, 7, 1))),
           lambda: orbx.ingest_batch_device(torch.as_strided(src, (2, 4, 8, 3), (95, 24, 3, 1)), out=out),
           lambda: orbx.ingest_batch_device(src, False, maps[:0].reshape(0, 4, 8), maps, out=out)]   # nmaps 0
    for k, call in enumerate(bad):
        with pytest.raises(orbx.OrbxError) as e:
            call()
        assert e.value.code == orbx.EINVAL, k
    with pytest.raises(orbx.OrbxError) as e:                                         # one map NULL, raw
        orbx._check("orbx_ingest_batch_device",
                    raw_ingest(orbx.lib, src=src.data_ptr(), batch=2, ch=3, mx=maps.data_ptr(), nmaps=1,
                               dst=out.data_ptr()))
    assert e.value.code == orbx.EINVAL
    assert raw_ingest(orbx.lib, src=src.data_ptr(), batch=0, ch=3, dst=out.data_ptr()) == orbx.OK
    assert raw_ingest(orbx.lib, src=src.data_ptr(), batch=0, ch=3, mx=maps.data_ptr(), my=maps.data_ptr(), nmaps=1,
                      dst=out.data_ptr()) == orbx.OK
    torch.cuda.synchronize()
    assert bool((out == DST_PAD).all())

"""k_describe's patch staging at every border class, with the bytes around the pixels as a test input.

k_describe (orb-slam-_amd/csrc/orbx_describe.hip) stages a keypoint's 43 x 43 patch by one of four paths, chosen
from (level, cx, cy, w, h, pitch): interior LDS-DMA; the same DMA for right-border keypoints, which reads up to 9
bytes past the row end; buffer-descriptor DMA for border keypoints of levels >= 1 with >= 16 bytes of row padding
(out-of-level bytes read as zeros and are repaired in LDS); reflect-101 bytes for the rest.  Three of them read
bytes that are not pixels.  Images of natural texture put a keypoint in most of these classes only by luck, so:

  atlas_image   a +-3 texture (below minThFAST: no corners of its own, but every blurred sample differs, so one
                wrong byte flips BRIEF bits) with small blobs placed where each level's border classes are;
  classify      the kernel's path choice restated (desc_patch_path), applied to the ORACLE's keypoints:
                test_atlas_covers_every_border_class is a condition on these inputs and runs without a GPU;
  GPU tests     each image through the host call (one keypoint per wave) and through batches of 10 (four per
                wave, border and interior keypoints sharing waves), tight and as a view into a sentinel-filled
                tensor with an odd pitch, in the three blur modes, each after orbx_debug_fill_workspace has set
                the row padding of the pyramid and of the staged image to 0x00, 0xFF and 0x5A.

Everything is compared bit-exactly through test_gpu_parity.assert_same_keypoints.
"""
import numpy as np
import pytest

NFEAT, SCALE, NLEVELS = 1000, 1.2, 4
# widths / row padding (align64) per level:
#   456 x 200: 456 380 317 264 / 56  4  3 56   byte-path levels 1, 2; buffer-path level 3
#   384 x 216: 384 320 267 222 /  0  0 53 34   zero-padding level 1 (right-border overruns land in the next row)
#   438 x 210: 438 365 304 253 / 10 19 16  3   w % 4 != 0; padding exactly 16; a byte-path last level
SIZES = [(456, 200), (384, 216), (438, 210)]
NVARIANTS = 10          # frames of a batch: the generator's variants 0..9
HOST_VARIANTS = (0, 1, 5)
FILLS = (0x00, 0xFF, 0x5A)
BLURS = (0, 1, 2)       # BLUR_SCALAR, BLUR_SSE2, BLUR_BITEXACT


def align64(w):
    return (w + 63) & ~63


def classify(level, cx, cy, w, h, pitch):
    """(path, sides) of a keypoint at (cx, cy) of a w x h level with `pitch` bytes per row: desc_patch_path of
    orbx_describe.hip restated.  sides: the level edges the 43 x 43 patch crosses, of "L" / "R" then "T" / "B"."""
    sides = ("L" if cx < 21 else "R" if cx + 21 >= w else "") + ("T" if cy < 21 else "B" if cy + 21 >= h else "")
    if cx >= 21 and cy >= 21 and cy + 21 < h and (cx + 31 <= w or (cx + 21 < w and cy + 22 < h)):
        return ("interior" if cx + 31 <= w else "right_dma"), sides
    if level > 0 and pitch - w >= 16 and not (cx < 21 and cy <= 21):
        return "buffer", sides
    return "byte", sides


def level_sizes(W, H):
    s = np.float32(1.0)
    out = []
    for _ in range(NLEVELS):
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
        s = np.float32(np.float64(s) * np.float64(np.float32(SCALE)))
    return out


def atlas_targets(w, h, level, v):
    """Level coordinates at which variant v asks for a keypoint of this level: along the four edges the two
    outermost keypoint positions (FAST keeps 19 px from the edge) alternate with their inner neighbours; the
    right edge alternates with the right-border DMA band cx in [w - 30, w - 22]; each corner steps through its
    2 x 3 positions with v; every other variant swaps the bottom-right corner for the band's cy = h - 22."""
    t = []
    o = (5 * level + 7 * v) % 18
    for i, y in enumerate(range(44 + o, h - 44, 18)):
        t.append((19 + (i + v) % 3, y))                                    # L, L, none
        t.append((w - 21 + (i + v) % 2 if i % 2 else w - 30 + (i // 2 + v + level) % 9, y))   # R | right-border DMA
    for i, x in enumerate(range(44 + o, w - 52, 18)):
        t.append((x, 19 + (i + v) % 3))
        t.append((x, h - 20 - (i + v) % 3))
    c = v >> 1
    t.append((19 + (v & 1), 19 + c % 3))
    t.append((w - 20 - (v & 1), 19 + c % 3))
    t.append((19 + (v & 1), h - 20 - c % 3))
    if v & 1:
        t.append((w - 30 + (c + level) % 9, h - 22))
    else:
        t.append((w - 20 - (c & 1), h - 20 - (c >> 1) % 3))
    return t


def atlas_image(W, H, v):
    """Variant v of the W x H atlas image (deterministic)."""
    rng = np.random.default_rng([W, H, v])
    img = (128 + rng.integers(-3, 4, (H, W))).astype(np.uint8)
    k = 0
    for level, (w, h) in enumerate(level_sizes(W, H)):
        for cx, cy in atlas_targets(w, h, level, v):
            val = (232, 24, 205, 60)[(k + v) % 4]
            k += 1
            if level == 0:
                img[cy, cx] = val   # a single pixel at level 0 is exactly that keypoint
                continue
            # the 2 x 2 block whose centre maps nearest to the level pixel's centre (cv::resize's mapping)
            bx, by = int(round((cx + 0.5) * W / w - 1.0)), int(round((cy + 0.5) * H / h - 1.0))
            img[by:by + 2, bx:bx + 2] = val
    return img


def keypoint_classes(kps, W, H, pitch0):
    """(level, path, sides, cx, cy, w, h, padding) of every oracle keypoint; level 0 rows are pitch0 bytes."""
    sizes = level_sizes(W, H)
    out = []
    s = [np.float32(1.0)]
    for _ in range(1, NLEVELS):
        s.append(np.float32(np.float64(s[-1]) * np.float64(np.float32(SCALE))))
    for kp in kps:
        l = int(kp["octave"])
        cx, cy = int(round(float(kp["x"]) / float(s[l]))), int(round(float(kp["y"]) / float(s[l])))
        w, h = sizes[l]
        pitch = pitch0 if l == 0 else align64(w)
        path, sides = classify(l, cx, cy, w, h, pitch)
        out.append((l, path, sides, cx, cy, w, h, pitch - w))
    return out


_refs = {}


def atlas_ref(orbref, W, H, v, blur=0):
    """The oracle's result for variant v (computed once per (size, variant, blur) and shared)."""
    key = (W, H, v, blur)
    if key not in _refs:
        p = orbref.make_params(NFEAT, SCALE, NLEVELS, 20, 7)
        _refs[key] = orbref.extract(atlas_image(W, H, v), p, want_pyramid=False, modes=(0, blur, 0))
    return _refs[key]


# ---- CPU: the inputs reach every class --------------------------------------------------------------------------
SIDES = ("L", "R", "T", "B", "LT", "RT", "LB", "RB")


def test_level_sizes_match_oracle(orbref):
    p = orbref.make_params(NFEAT, SCALE, NLEVELS, 20, 7)
    for W, H in SIZES:
        assert level_sizes(W, H) == orbref.level_sizes(p, W, H)
    assert [w for w, _ in level_sizes(456, 200)] == [456, 380, 317, 264]
    assert [w for w, _ in level_sizes(384, 216)] == [384, 320, 267, 222]
    assert [w for w, _ in level_sizes(438, 210)] == [438, 365, 304, 253]


def test_atlas_covers_every_border_class(orbref):
    """The oracle's keypoints of the atlas images, over all sizes and variants (tight level-0 rows), fall in every
    class of k_describe's path choice.  A condition on the test inputs: the GPU tests below compare exactly these
    keypoints' descriptors."""
    seen = set()
    for W, H in SIZES:
        for v in range(NVARIANTS):
            ref = atlas_ref(orbref, W, H, v)
            for l, path, sides, cx, cy, w, h, pad in keypoint_classes(ref.keypoints, W, H, W):
                kind = "level 0" if l == 0 else "padded" if pad >= 16 else "unpadded"
                if path in ("buffer", "byte") and sides:
                    seen.add((path, kind, sides))
                    if path == "buffer" and sides == "RB" and l == NLEVELS - 1:
                        seen.add(("buffer", "last level", "RB"))   # the pieces at the descriptor's end
                # the keypoints whose 16-byte piece of level row 0 would start at offset -4 of a buffer
                # descriptor: desc_patch_path sends them to the byte path
                if kind == "padded" and cx < 21 and cy <= 21:
                    assert path == "byte"
                    seen.add(("negative offset", "cx", cx))
                    seen.add(("negative offset", "cy", "21" if cy == 21 else "<21"))
                if path == "right_dma" and l > 0:
                    seen.add(("right_dma", "padding >= 9" if pad >= 9 else "padding < 9"))
                if cy == h - 22 and cx + 21 < w < cx + 31:   # one row too low for the right-border DMA
                    assert path in ("buffer", "byte") and not sides
                    seen.add(("right_dma neighbour", path))
                if path == "interior":
                    seen.add(("interior",))
    # (a padded level's top-left corner is the negative-offset class: byte path, never the buffer path)
    assert ("buffer", "padded", "LT") not in seen and not any(k[:2] == ("buffer", "unpadded") for k in seen)
    want = {("buffer", "padded", s) for s in SIDES if s != "LT"} | {("buffer", "last level", "RB")}
    want |= {("byte", "padded", "LT")}
    want |= {("byte", "unpadded", s) for s in SIDES} | {("byte", "level 0", s) for s in SIDES}
    want |= {("negative offset", "cx", 19), ("negative offset", "cx", 20),
             ("negative offset", "cy", "21"), ("negative offset", "cy", "<21")}
    want |= {("right_dma", "padding >= 9"), ("right_dma", "padding < 9"), ("interior",)}
    want |= {("right_dma neighbour", "buffer"), ("right_dma neighbour", "byte")}
    missing = sorted(want - seen, key=str)
    assert not missing, missing


# ---- GPU: every class, bit-exact, whatever the bytes around the pixels hold -----------------------------------------
def _extractor(blur, nlevels=NLEVELS):
    import orbx
    ex = orbx.ORBextractor(NFEAT, SCALE, nlevels, 20, 7)
    ex.set_cv_modes(0, blur)
    return ex


def _batch_rounds(ex, frames, cuda, view):
    """Yields (tag, keypoints, descriptors) of the batch: once to size the workspace, then after each byte-fill
    of it (the workspace only grows, so the second extraction of a shape keeps the fill in every byte the
    pyramid kernels do not write).  view: the frames sit in a larger tensor, rows at a pitch that is no multiple
    of 4 and gap rows between frames, and everything around them holds a sentinel that changes with the fill."""
    import torch
    import orbx
    B, H, W = frames.shape
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(cuda)
    cap = ex.capacity(H, W)
    kps = torch.empty((B, cap, 7), dtype=torch.int32, device=cuda)
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=cuda)
    counts = torch.empty((B,), dtype=torch.int32, device=cuda)
    big = torch.empty((B, H + 3, W + 13), dtype=torch.uint8, device=cuda)
    assert (W + 13) % 4 != 0
    for fill in (None,) + FILLS:
        if fill is not None:
            ex.debug_fill_workspace(fill)
        if view:
            big.fill_(0x3C if fill is None else 0xFF - fill)
            imgs = big[:, 1:H + 1, 5:5 + W]
            imgs.copy_(src)
            assert imgs.stride(1) == W + 13 and imgs.stride(0) == (H + 3) * (W + 13)
        else:
            imgs = src
        kps.zero_()
        desc.zero_()
        ex.extract_batch_device(imgs, kps, desc, counts)
        ex.sync(torch.cuda.current_stream())
        c = counts.cpu().numpy()
        d = desc.cpu().numpy()
        yield ("sizing run" if fill is None else "fill 0x%02X" % fill), orbx.keypoints_from_device(kps, counts), \
            [d[f, :c[f]] for f in range(B)]


@pytest.mark.gpu
@pytest.mark.parametrize("blur", BLURS)
@pytest.mark.parametrize("W,H", SIZES)
def test_atlas_host_call(orbref, cuda, W, H, blur):
    """The single-frame host call (one keypoint per describe wave; rows staged at align64(W))."""
    from test_gpu_parity import assert_same_keypoints
    ex = _extractor(blur)
    for v in HOST_VARIANTS:
        img = atlas_image(W, H, v)
        ref = atlas_ref(orbref, W, H, v, blur)
        for fill in (None,) + FILLS:
            if fill is not None:
                ex.debug_fill_workspace(fill)
            kps, desc = ex(img)
            assert_same_keypoints(kps, ref.keypoints, desc, ref.descriptors,
                                  "%dx%d v%d blur %d host %s" % (W, H, v, blur, fill))


@pytest.mark.gpu
@pytest.mark.parametrize("blur", BLURS)
@pytest.mark.parametrize("view", [False, True], ids=["tight", "view"])
@pytest.mark.parametrize("W,H", SIZES)
def test_atlas_batch(orbref, cuda, W, H, view, blur):
    """A batch of the 10 variants: four keypoints per describe wave, so border and interior keypoints share waves
    and the patch prefetch and its wait count hand over between the staging paths."""
    from test_gpu_parity import assert_same_keypoints
    frames = np.stack([atlas_image(W, H, v) for v in range(NVARIANTS)])
    ex = _extractor(blur)
    for tag, klist, dlist in _batch_rounds(ex, frames, cuda, view):
        for v in range(NVARIANTS):
            ref = atlas_ref(orbref, W, H, v, blur)
            assert_same_keypoints(klist[v], ref.keypoints, dlist[v], ref.descriptors,
                                  "%dx%d v%d blur %d %s %s" % (W, H, v, blur, "view" if view else "tight", tag))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", 2, 10])
def test_tum_padding_fills(orbref, cuda, mode):
    """test_gpu_parity's tum640 frames (8 levels; level 2 is 444 px in a 448-byte pitch, the shape whose border
    descriptors once depended on the row padding) with the padding filled."""
    from test_gpu_parity import _frames, assert_same_keypoints
    p = orbref.make_params(NFEAT, SCALE, 8, 20, 7)
    frames = _frames("gen", 640, 480, 1 if mode == "host" else mode)
    refs = [orbref.extract(f, p, want_pyramid=False) for f in frames]
    ex = _extractor(0, 8)
    if mode == "host":
        for fill in (None,) + FILLS:
            if fill is not None:
                ex.debug_fill_workspace(fill)
            kps, desc = ex(frames[0])
            assert_same_keypoints(kps, refs[0].keypoints, desc, refs[0].descriptors, "tum host %s" % fill)
        return
    for tag, klist, dlist in _batch_rounds(ex, frames, cuda, False):
        for f in range(len(frames)):
            assert_same_keypoints(klist[f], refs[f].keypoints, dlist[f], refs[f].descriptors,
                                  "tum b%s f%d %s" % (mode, f, tag))

"""Raw Oxford RobotCar frames: bilinear Bayer demosaic and look-up-table undistortion.

The released models were trained on frames made by the reference's
``prepare_data/001_downsize_images.py``: ``oxford_image.load_image(file, cam)`` of the RobotCar SDK
(bilinear demosaic, the camera model's undistortion, ``astype(uint8)``), then ``resize_img(img, 240)``.
A frame straight from the Bumblebee centre camera is a 960 x 1280 one-channel Bayer mosaic ('gbrg').

THE SDK AND ``colour_demosaicing`` ARE NOT INSTALLED where this was written.  What is stated here is
the SDK's chain as recalled (SDK 2.1: ``demosaicing_CFA_Bayer_bilinear`` = three masked planes through
``scipy.ndimage.convolve`` with its default border ``mode='reflect'``; ``CameraModel.undistort`` =
``scipy.ndimage.map_coordinates(order=1)`` per channel with the file ``<camera>_distortion_lut.bin``;
``np.array(img).astype(np.uint8)``) — UNVERIFIED against the SDK itself.  The mathematics is pinned
against the scipy functions the SDK calls (tests/test_robotcar_host.py: equal bit for bit in float64
and in the bytes), not against a transcription of the SDK.

The definition (``load_image_np``; on the device csrc/frames.hip ``scl_frames_debayer``,
util/device_cv.py ``DeviceResizer.debayer``):

  demosaic    q[c][y][x] = sum over the 3 x 3 taps of k_c * (raw where the site has colour c, else 0),
              in integers, with 4 H_G = [[0,1,0],[1,4,1],[0,1,0]] and 4 H_RB = [[1,2,1],[2,4,2],[1,2,1]];
              the value is q / 4 in float64 (exact).  Outside the frame ``border='reflect'`` reads
              index -1 -> 0 and n -> n-1 (scipy's default, ``d c b a | a b c d``), ``'mirror'`` reads
              -1 -> 1 and n -> n-2.  The colour of a tap is the colour of the site it READS.
  undistort   per pixel with ``ly, lx`` from the table: outside ``0 <= ly <= SH-1, 0 <= lx <= SW-1``
              (a NaN is outside) the value is 0.0; inside, y0 = floor(ly), ty = ly - y0, wy0 = 1 - ty
              (the same for x), y1 = min(y0 + 1, SH-1), x1 = min(x0 + 1, SW-1) and
              acc = 0.0; acc += (v[y0,x0]*wy0)*wx0; acc += (v[y0,x1]*wy0)*tx; acc += (v[y1,x0]*ty)*wx0;
              acc += (v[y1,x1]*ty)*tx — every operation a float64 operation rounded on its own.
  byte        acc truncated toward zero, then the low 8 bits: ``acc.astype(np.int64).astype(np.uint8)``.

UNDER 'reflect' THE BORDER WRAPS: the reflected index doubles the border rows and columns of the
masked planes, so a demosaiced value at the border reaches 573.75 on an all-255 frame (2.25 x), and the
byte keeps its low 8 bits (573 -> 61).  That is the SDK's behaviour if the recollection of the default
border holds; 'mirror' stays within 0..255.  The border rule is a parameter so that someone with the
SDK can settle it without new device code.

    python -m soft_contrastive_learning_amd.util.robotcar --in_dir D --out_dir O --distortion_lut F
           [--pattern gbrg --border reflect --max_side 240 --batch 16]

is ``001_downsize_images.py`` for a directory tree of raw PNGs on the device (tar archives are not
read): ``O/<same relative path>.png`` and ``O/exposure.csv`` with the columns ``path`` and ``exposure``
(the integer sum of the resized frame's bytes).  An unreadable PNG is skipped and listed.
"""
import os

import numpy as np

PATTERNS = ('rggb', 'bggr', 'grbg', 'gbrg')     # index = the `pattern` argument of scl_frames_debayer
STEREO_PATTERN = 'gbrg'                         # Bumblebee XB3 (stereo/left, centre, right)
MONO_PATTERN = 'rggb'                           # Grasshopper2 (mono_left, mono_right, mono_rear)
BORDERS = ('reflect', 'mirror')                 # index = the `border` argument

_K4_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=np.int64)
_K4_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.int64)


def pattern_index(pattern):
    p = str(pattern).lower()
    if p not in PATTERNS:
        raise ValueError('pattern is one of %s, not %r' % (', '.join(PATTERNS), pattern))
    return PATTERNS.index(p)


def border_index(border):
    if border not in BORDERS:
        raise ValueError("border is 'reflect' or 'mirror', not %r" % (border,))
    return BORDERS.index(border)


def masks(sh, sw, pattern):
    """bool [3, sh, sw]: the sites of R, G and B.  The characters of the pattern fall on the sites
    (0,0), (0,1), (1,0), (1,1) of every 2 x 2 cell, in that order."""
    p = PATTERNS[pattern_index(pattern)]
    m = np.zeros((3, sh, sw), dtype=bool)
    for ch, (y, x) in zip(p, ((0, 0), (0, 1), (1, 0), (1, 1))):
        m['rgb'.index(ch), y::2, x::2] = True
    return m


def _as_raw(raw):
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim != 2 or raw.shape[0] < 2 or raw.shape[1] < 2:
        raise ValueError('a raw frame is uint8 [SH, SW] with both sides at least 2, not %s %s'
                         % (raw.dtype, raw.shape))
    return raw


def demosaic_quarters(raw, pattern=STEREO_PATTERN, border='reflect'):
    """int64 [SH, SW, 3]: the demosaiced frame in quarter units (exact)."""
    raw = _as_raw(raw)
    sh, sw = raw.shape
    mirror = border_index(border) == 1
    # the padded index maps: position -1 .. n of the frame -> the index read
    ys = np.concatenate(([1 if mirror else 0], np.arange(sh), [sh - 2 if mirror else sh - 1]))
    xs = np.concatenate(([1 if mirror else 0], np.arange(sw), [sw - 2 if mirror else sw - 1]))
    q = np.zeros((sh, sw, 3), dtype=np.int64)
    for c, m in enumerate(masks(sh, sw, pattern)):
        plane = np.where(m, raw, 0).astype(np.int64)[ys][:, xs]          # [sh + 2, sw + 2]
        k = _K4_G if c == 1 else _K4_RB
        for dy in range(3):
            for dx in range(3):
                if k[dy, dx]:
                    q[:, :, c] += k[dy, dx] * plane[dy:dy + sh, dx:dx + sw]
    return q


def demosaic_np(raw, pattern=STEREO_PATTERN, border='reflect'):
    """float64 [SH, SW, 3] (R, G, B): ``demosaicing_CFA_Bayer_bilinear`` as stated above."""
    return demosaic_quarters(raw, pattern, border) / 4.0


def identity_lut(sh, sw):
    """float64 [2, sh*sw]: every pixel reads itself."""
    yy, xx = np.mgrid[0:sh, 0:sw]
    return np.stack([xx.ravel(), yy.ravel()]).astype(np.float64)


def undistort_np(img, lut):
    """float64 image [SH, SW] or [SH, SW, C] sampled at the table's coordinates: float64 of the same
    shape.  ``lut`` is float64 [2, SH*SW]: the column coordinate of every pixel, then the row
    coordinate (the layout of ``<camera>_distortion_lut.bin``)."""
    img = np.asarray(img, dtype=np.float64)
    flat = img.ndim == 2
    v = img[:, :, None] if flat else img
    sh, sw = v.shape[:2]
    lut = np.asarray(lut, dtype=np.float64)
    if lut.shape != (2, sh * sw):
        raise ValueError('Incorrect image size for camera model: the table is %s, the image %d x %d'
                         % (lut.shape, sh, sw))
    lx, ly = lut[0].reshape(sh, sw), lut[1].reshape(sh, sw)
    with np.errstate(invalid='ignore'):
        inside = (ly >= 0) & (ly <= sh - 1) & (lx >= 0) & (lx <= sw - 1)
    ly, lx = np.where(inside, ly, 0.0), np.where(inside, lx, 0.0)
    fy, fx = np.floor(ly), np.floor(lx)
    ty, tx = ly - fy, lx - fx
    wy0, wx0 = 1.0 - ty, 1.0 - tx
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
    ty, tx, wy0, wx0 = ty[..., None], tx[..., None], wy0[..., None], wx0[..., None]
    acc = np.zeros(v.shape, dtype=np.float64)
    acc += (v[y0, x0] * wy0) * wx0
    acc += (v[y0, x1] * wy0) * tx
    acc += (v[y1, x0] * ty) * wx0
    acc += (v[y1, x1] * ty) * tx
    acc = np.where(inside[..., None], acc, 0.0)
    return acc[:, :, 0] if flat else acc


def to_bytes(acc):
    """Truncate toward zero, keep the low 8 bits (values above 255 wrap: see the module's text)."""
    return np.asarray(acc).astype(np.int64).astype(np.uint8)


def load_image_np(raw, pattern=STEREO_PATTERN, lut=None, border='reflect'):
    """uint8 [SH, SW, 3]: the SDK's ``load_image`` of a raw frame — demosaic, undistort (``lut`` None:
    skipped, like a call without a camera model), byte."""
    img = demosaic_np(raw, pattern, border)
    if lut is not None:
        img = undistort_np(img, lut)
    return to_bytes(img)


def load_distortion_lut(path, sh, sw):
    """``<camera>_distortion_lut.bin`` -> float64 [2, sh*sw] (column coordinates, row coordinates)."""
    lut = np.fromfile(str(path), dtype=np.float64)
    if lut.size != 2 * int(sh) * int(sw):
        raise ValueError('Incorrect image size for camera model: %s holds %d float64, a %d x %d frame '
                         'needs %d' % (path, lut.size, sh, sw, 2 * int(sh) * int(sw)))
    return np.ascontiguousarray(lut.reshape(2, int(sh) * int(sw)))


def save_distortion_lut(lut, path):
    np.ascontiguousarray(lut, dtype=np.float64).tofile(str(path))


# ---- the reference's 001_downsize_images.py for a directory tree -------------------------------------
def load_raw_png(path):
    """A one-channel 8-bit PNG as uint8 [SH, SW]; ValueError for anything else."""
    from PIL import Image
    with Image.open(str(path)) as im:
        if im.mode != 'L':
            raise ValueError('%s is a %s image; a raw Bayer frame has one 8-bit channel' % (path, im.mode))
        return np.asarray(im, dtype=np.uint8)


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m soft_contrastive_learning_amd.util.robotcar')
    p.add_argument('--in_dir', required=True, help='tree of raw one-channel PNGs')
    p.add_argument('--out_dir', required=True)
    p.add_argument('--distortion_lut', required=True, help='<camera>_distortion_lut.bin of the SDK')
    p.add_argument('--pattern', default=STEREO_PATTERN, choices=list(PATTERNS))
    p.add_argument('--border', default='reflect', choices=list(BORDERS))
    p.add_argument('--max_side', default=240, type=int)
    p.add_argument('--batch', default=16, type=int)
    return p


def _flush(resizer, group, lut, flags, rows):
    """One device call for the frames of ``group`` [(relative path, raw)], all of one shape."""
    import torch

    from . import io
    out = resizer.debayer([raw for _, raw in group], flags.pattern, lut, flags.border, 'resize_img',
                          torch.uint8, max_size=flags.max_side)
    exposure = out.sum(dim=(1, 2, 3), dtype=torch.int64).cpu().numpy()
    for (rel, _), img, e in zip(group, out.cpu().numpy(), exposure):
        dst = os.path.join(flags.out_dir, rel)
        os.makedirs(os.path.dirname(dst) or '.', exist_ok=True)
        io.save_img(img, dst)
        rows.append((rel, int(e)))


def main(argv=None):
    """Returns (rows written [(relative path, exposure)], skipped [relative path])."""
    flags = build_parser().parse_args(argv)
    if not os.path.isdir(flags.in_dir):
        raise SystemExit('--in_dir %s is no directory' % flags.in_dir)
    if not os.path.isfile(flags.distortion_lut):
        raise SystemExit('--distortion_lut %s does not exist' % flags.distortion_lut)
    if flags.max_side < 1 or flags.batch < 1:
        raise SystemExit('--max_side and --batch are at least 1')
    if os.path.abspath(flags.in_dir) == os.path.abspath(flags.out_dir):
        raise SystemExit('--out_dir is --in_dir: the raw frames would be overwritten')
    rels = sorted(os.path.relpath(os.path.join(d, f), flags.in_dir)
                  for d, _, files in os.walk(flags.in_dir) for f in files if f.lower().endswith('.png'))
    if not rels:
        raise SystemExit('no .png under %s' % flags.in_dir)
    from . import io
    from .device_cv import DeviceResizer
    resizer = DeviceResizer('cuda')
    rows, skipped, group, lut, shape = [], [], [], None, None
    for rel in rels:
        try:
            raw = load_raw_png(os.path.join(flags.in_dir, rel))
        except Exception as e:                        # the reference skips what it cannot read
            print('skipped %s: %s' % (rel, e))
            skipped.append(rel)
            continue
        if lut is None:                               # the first readable frame names the camera's size
            try:
                lut, shape = load_distortion_lut(flags.distortion_lut, *raw.shape), raw.shape
            except ValueError as e:
                raise SystemExit(str(e))
        if raw.shape != shape:
            print('skipped %s: %d x %d is not the camera model\'s size' % (rel, raw.shape[1], raw.shape[0]))
            skipped.append(rel)
            continue
        group.append((rel, raw))
        if len(group) == flags.batch:
            _flush(resizer, group, lut, flags, rows)
            group = []
    if group:
        _flush(resizer, group, lut, flags, rows)
    os.makedirs(flags.out_dir, exist_ok=True)
    io.save_csv({'path': [r for r, _ in rows], 'exposure': [e for _, e in rows]},
                os.path.join(flags.out_dir, 'exposure.csv'))
    print('wrote %d frames to %s, skipped %d' % (len(rows), flags.out_dir, len(skipped)))
    for rel in skipped:
        print('  skipped:', rel)
    return rows, skipped


if __name__ == '__main__':
    main()

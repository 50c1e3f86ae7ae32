"""Shared inputs of tests/test_robotcar_host.py and tests/test_gpu_robotcar_raw.py: raw Bayer frames and
distortion tables with every kind of coordinate the definition of util/robotcar.py distinguishes."""
import numpy as np

from soft_contrastive_learning_amd.util import robotcar

SHAPES = [(2, 2), (3, 5), (6, 8), (7, 9), (96, 128)]          # 6 x 8 is the all-255 frame
CASES = [(sh, sw, p, b) for sh, sw in SHAPES for p in robotcar.PATTERNS for b in robotcar.BORDERS]


def raw_frames(n, sh, sw, seed=0):
    """uint8 [n, sh, sw]; the frames of a batch differ.  6 x 8: frame 0 is all 255 (the wrap at the
    'reflect' border: 573.75 -> 61)."""
    raw = np.random.default_rng(1000 * sh + sw + seed).integers(0, 256, size=(n, sh, sw), dtype=np.uint8)
    if (sh, sw) == (6, 8):
        raw[0] = 255
    return raw


def mixed_lut(sh, sw, seed=0):
    """float64 [2, sh*sw]: identity +- 1.5 px (so some coordinates leave the frame), a quarter of them
    rounded to integers, and the exact edge coordinates, a negative zero, a coordinate one part in
    10^12 past the edge and NaN written over the first pixels (cyclically on tiny frames)."""
    rng = np.random.default_rng(77 * sh + sw + seed)
    lut = robotcar.identity_lut(sh, sw) + rng.uniform(-1.5, 1.5, size=(2, sh * sw))
    whole = rng.random((2, sh * sw)) < 0.25
    lut[whole] = np.rint(lut[whole])
    npix = sh * sw
    special = [(sh - 1.0, 0.5), (0.0, sw - 1.0), (-0.0, -0.0), (sh - 1 + 1e-12, 0.0), (0.5, sw - 1 + 1e-12),
               (np.nan, 0.0), (1.0, np.nan), (sh - 1.0, sw - 1.0), (sh - 1.5, sw - 1.5), (-1e-12, 0.0)]
    # spread over the frame on the larger shapes, so the 2 x 2 .. 7 x 9 frames keep random entries too
    step = max(npix // (len(special) + 1), 1)
    for k, (ly, lx) in enumerate(special if npix > 12 else special[seed % 5::5]):
        lut[1, (k * step + 1) % npix], lut[0, (k * step + 1) % npix] = ly, lx
    return lut


def smooth_lut(sh, sw, seed=0):
    """A lens-like table: scale 0.9 about the centre, an offset, noise below 1 px."""
    rng = np.random.default_rng(seed)
    ident = robotcar.identity_lut(sh, sw)
    cx, cy = (sw - 1) / 2.0, (sh - 1) / 2.0
    lx = cx + 0.9 * (ident[0] - cx) + 3.25 + rng.uniform(-0.9, 0.9, sh * sw)
    ly = cy + 0.9 * (ident[1] - cy) - 2.5 + rng.uniform(-0.9, 0.9, sh * sw)
    return np.stack([lx, ly])

"""Feature-extraction counterpart of the reference's ``evaluation/inference.py``.

Reproduces ``infer()`` (evaluation/inference.py:147-192): the image list is padded with
copies of image 0 up to a multiple of ``images_per_pass`` (:172-175), batches go through
``vgg16Netvlad`` forward-only (:89-90, :46), results are re-ordered by original index,
padding rows are dropped (:186-191) and the product is a pickle holding a ``list`` of
``np.ndarray(32768,) float32`` in list order (:192).

Images: ``--csv_root/<set>.csv`` with a ``path`` column relative to ``--img_root``
(evaluation/inference.py:168-170), decoded and sized by ``load_images``' rules (:52-72; util/cv.py,
util/io.py restated in ``soft_contrastive_learning_amd/util``): 'oxs' sets read ``.jpg`` instead of
``.png``, 'achen' sets are portrait (cover ``large_side x small_side``), with the NetVLAD head the
longer side becomes ``large_side`` unless ``--rescale`` is off, without it the frame is brought to
``small_side x large_side``.  Six loader threads feed the device (:155-160).  ``--set synthetic``:
random images, no files.  ``--device_resize 1`` leaves the sizing of the decoded frames to the device
(util/device_cv.py, csrc/frames.hip: the same pixels, the same pickle).  ``--bayer PATTERN
--distortion_lut FILE [--bayer_border reflect|mirror]`` (they need ``--device_resize 1``): the files are
raw one-channel Bayer frames as the RobotCar cameras deliver them; the device demosaics, undistorts and
sizes them in one launch (util/robotcar.py states what is computed; the SDK it restates was not available).
"""
import argparse
import os
import pickle

import numpy as np
import torch

from .. import checkpoint
from ..model import nets, reduction


def pad_indices(num, images_per_pass):
    """evaluation/inference.py:172-175 — note the reference pads a FULL extra pass when
    ``num`` is already a multiple (``images_per_pass - num % images_per_pass``)."""
    padding = [0] * (images_per_pass - (num % images_per_pass))
    return np.concatenate((np.arange(num), np.array(padding, dtype=int))).astype(int)


def size_on_host(img, rule, kw):
    """One decoded frame through a sizing rule of ``csv_loader`` on the host (util/cv.py)."""
    from ..util import cv
    if rule == 'none':
        return img
    return getattr(cv, rule)(img, **kw)


def extract_features(model, loader, num, images_per_pass=4, device=None, loader_threads=6,
                     device_resize=False, debayer=None):
    """Returns ``list`` of ``num`` float32 vectors (length 32768 with the NetVLAD head, H' W' 512
    without: ``ops['full_out']``, evaluation/inference.py:89-92; ``out_dim`` with a dense reduction
    head: ``ops['output']``, :97-109), in index order.  ``loader`` is
    called from ``loader_threads`` threads (cpu_thread, :28-38), one batch ahead of the device.

    ``device_resize``: ``loader`` returns ``(decoded uint8 frame, rule, parameters)``
    (``csv_loader(device_resize=True)``) and every batch is sized on the device
    (util/device_cv.py: the host's pixels bit for bit).  A batch whose frames do not share one
    source shape is sized on the host, frame by frame, as without the flag; such batches are
    counted and the count is printed at the end.

    ``debayer`` = (pattern, lut, border) with ``device_resize``: the decoded frames are raw Bayer
    mosaics [SH,SW] (``csv_loader(bayer=...)``) and go through ``DeviceResizer.debayer``; on the host
    route of a mixed batch through ``robotcar.load_image_np`` (a frame the table does not fit raises)."""
    from concurrent.futures import ThreadPoolExecutor
    device = device or next(model.parameters()).device
    order = pad_indices(num, images_per_pass)
    feats = [None] * len(order)
    starts = list(range(0, len(order), images_per_pass))

    def load_batch(s):
        idx = order[s:s + images_per_pass]
        if not device_resize:
            return np.stack([np.asarray(loader(int(i)), dtype=np.float32) for i in idx])
        raw = [loader(int(i)) for i in idx]
        if len({(img.shape, rule, tuple(sorted(kw.items()))) for img, rule, kw in raw}) == 1:
            return np.stack([img for img, _, _ in raw]), raw[0][1], raw[0][2]
        if debayer is not None:
            from ..util import robotcar
            raw = [(robotcar.load_image_np(img, *debayer), rule, kw) for img, rule, kw in raw]
        return np.stack([np.asarray(size_on_host(*r), dtype=np.float32) for r in raw])
    on_host = 0                       # batches of mixed source shapes (device_resize only)
    if device_resize:
        from ..util.device_cv import DeviceResizer
        resizer = DeviceResizer(device)
    with torch.no_grad(), ThreadPoolExecutor(max_workers=max(int(loader_threads), 1)) as pool:
        ahead = max(int(loader_threads), 1)
        pending = [pool.submit(load_batch, s) for s in starts[:ahead]]
        for k, s in enumerate(starts):
            batch = pending.pop(0).result()
            if k + ahead < len(starts):
                pending.append(pool.submit(load_batch, starts[k + ahead]))
            if isinstance(batch, tuple):
                frames, rule, kw = batch
                if debayer is not None:
                    batch = resizer.debayer(frames, debayer[0], debayer[1], debayer[2], rule, torch.float32, **kw)
                else:
                    batch = resizer.apply(frames, rule, torch.float32, **kw)
            else:
                on_host += int(device_resize)
                batch = torch.from_numpy(batch).to(device)
            out = nets.output(batch, model=model)
            out = out.float().cpu().numpy()
            for slot, f in zip(range(s, s + len(out)), out):
                feats[slot] = f
    if device_resize:
        print('device_resize: {} of {} batches sized on the host (mixed source shapes)'.format(
            on_host, len(starts)))
    return feats[:num]


def csv_loader(set_name, csv_root, img_root, vlad_cores=64, rescale=True, small_side=180, large_side=240,
               device_resize=False, bayer=''):
    """(loader, num) over ``<csv_root>/<set>.csv`` (column ``path``): evaluation/inference.py:52-72,
    168-170.  ``device_resize``: the loader returns ``(decoded uint8 frame, rule, parameters)`` —
    the frame as decoded and the sizing it would have applied (``size_on_host``,
    ``DeviceResizer.apply``) — for ``extract_features(device_resize=True)``.  ``bayer`` (a pattern;
    needs ``device_resize``): the files are raw Bayer frames and are returned as decoded, uint8 [SH,SW];
    a file with more than one channel raises."""
    from ..util import io
    if bayer and not device_resize:
        raise ValueError('raw Bayer frames (bayer=%r) are prepared on the device: device_resize=True' % (bayer,))
    meta = io.load_csv(os.path.join(csv_root, '{}.csv'.format(set_name)))
    if not isinstance(meta, dict) or 'path' not in meta:
        raise ValueError('%s.csv needs a "path" column and at least one row' % set_name)
    paths = list(meta['path'])

    def load(i):
        rel = paths[i]
        if 'oxs' in set_name:
            rel = rel.replace('.png', '.jpg')
        if bayer:
            from ..util import robotcar
            img = robotcar.load_raw_png(os.path.join(img_root, rel))
        else:
            img = io.load_img(os.path.join(img_root, rel))
        return (img, rule, kw) if device_resize else size_on_host(img, rule, kw)
    if 'achen' in set_name:
        rule, kw = 'standard_size', dict(h=large_side, w=small_side)        # portrait images
    elif vlad_cores > 0:
        rule, kw = ('resize_img', dict(max_size=large_side)) if rescale else ('none', {})
    else:
        rule, kw = 'standard_size', dict(h=small_side, w=large_side)
    return load, len(paths)


def save_pickle(data, out_file):
    with open(out_file, 'wb') as f:
        pickle.dump(data, f)


def synthetic_loader(height, width, seed=42):
    def load(i):
        rng = np.random.default_rng(seed + i)
        return rng.integers(0, 256, size=(height, width, 3)).astype(np.float32)
    return load


def build_parser():
    p = argparse.ArgumentParser()
    # flag names of evaluation/inference.py:204-230
    p.add_argument('--rescale', default=True,
                   type=lambda v: str(v).lower() not in ('0', 'false', 'no', ''))
    p.add_argument('--small_side', default=180, type=int)
    p.add_argument('--large_side', default=240, type=int)
    p.add_argument('--img_root', default='')
    p.add_argument('--csv_root', default='')
    p.add_argument('--set', default='synthetic')
    p.add_argument('--checkpoint', default='')
    p.add_argument('--out_name', default='scl_amd')
    p.add_argument('--out_dim', default=512, type=int)
    p.add_argument('--reduction', default='none', help='none, 1fc, 2fc, 3fc, pca')
    p.add_argument('--vlad_cores', default=64, type=int)
    p.add_argument('--out_root', default='./scl_lv')
    p.add_argument('--images_per_pass', type=int, default=4)
    p.add_argument('--num_images', type=int, default=10, help='synthetic set size')
    p.add_argument('--device_resize', type=int, default=0,
                   help='1: size the decoded frames of a CSV set on the device (csrc/frames.hip; '
                        'the pickle is the same)')
    p.add_argument('--bayer', default='',
                   help='the files are raw one-channel Bayer frames of this pattern (gbrg: RobotCar stereo, rggb: '
                        'mono); needs --device_resize 1 and --distortion_lut')
    p.add_argument('--distortion_lut', default='', help='<camera>_distortion_lut.bin of the RobotCar SDK')
    p.add_argument('--bayer_border', default='reflect', choices=['reflect', 'mirror'],
                   help="what the demosaic reads outside the frame (util/robotcar.py; 'reflect' is scipy's default)")
    return p


def raw_route(flags):
    """--bayer / --distortion_lut / --bayer_border checked against the other flags, before any device
    work: (pattern, table file, border), or None without --bayer."""
    from ..util import robotcar
    if not flags.bayer and not flags.distortion_lut:
        return None
    if not flags.bayer:
        raise SystemExit('--distortion_lut belongs to --bayer PATTERN (one of %s)' % ', '.join(robotcar.PATTERNS))
    if flags.bayer not in robotcar.PATTERNS:
        raise SystemExit('--bayer is one of %s, not %r' % (', '.join(robotcar.PATTERNS), flags.bayer))
    if not flags.device_resize:
        raise SystemExit('--bayer prepares the raw frames on the device: it needs --device_resize 1')
    if flags.set == 'synthetic' and not flags.csv_root:
        raise SystemExit('--bayer reads the files of a CSV set (--set, --csv_root, --img_root)')
    if not flags.distortion_lut:
        raise SystemExit('--bayer needs --distortion_lut FILE (the camera model\'s look-up table)')
    if not os.path.isfile(flags.distortion_lut):
        raise SystemExit('--distortion_lut %s does not exist' % flags.distortion_lut)
    return flags.bayer, flags.distortion_lut, flags.bayer_border


def main(argv=None):
    flags = build_parser().parse_args(argv)
    # --reduction pca writes the RAW descriptors, like the reference: "Don't actually do PCA
    # here - doing it after" (evaluation/inference.py:94-95; its projection branch at :111-116
    # is unreachable).  The whitening runs in evaluation/top_n.py.
    if flags.vlad_cores not in (0, 64) or flags.reduction not in ('none', 'pca') + reduction.KINDS:
        raise SystemExit('only --vlad_cores 64 | 0 with --reduction none|pca|1fc|2fc|3fc is on the hot path')
    raw = raw_route(flags)
    np.random.seed(42)                                       # inference.py:270-271
    model = nets.VGG16NetVLAD(vlad_cores=flags.vlad_cores).cuda()
    if flags.reduction in reduction.KINDS:
        # :97-109; the input of the head without NetVLAD is the fixed small_side x large_side frame
        # (:78-86)
        reduction.attach(model, flags.reduction, flags.out_dim, height=flags.small_side,
                         width=flags.large_side)
    if flags.checkpoint:
        checkpoint.load(model, flags.checkpoint)     # every variable, the head included (:122-131)
    device_resize = False
    if flags.set == 'synthetic' and not flags.csv_root:
        loader, num = synthetic_loader(flags.small_side, flags.large_side), flags.num_images
    else:
        device_resize = bool(flags.device_resize)
        loader, num = csv_loader(flags.set, flags.csv_root, flags.img_root, flags.vlad_cores,
                                 flags.rescale, flags.small_side, flags.large_side,
                                 device_resize=device_resize, bayer=raw[0] if raw else '')
    debayer = None
    if raw:
        from ..util import robotcar
        first = loader(0)[0]                              # the table is for the camera's frame size
        debayer = (raw[0], robotcar.load_distortion_lut(raw[1], *first.shape), raw[2])
    feats = extract_features(model, loader, num, flags.images_per_pass, device_resize=device_resize,
                             debayer=debayer)
    os.makedirs(flags.out_root, exist_ok=True)
    out = os.path.join(flags.out_root, '{}_{}.pickle'.format(flags.set, flags.out_name))
    save_pickle(feats, out)
    print('wrote', out, len(feats), feats[0].shape, feats[0].dtype)


if __name__ == '__main__':
    main()

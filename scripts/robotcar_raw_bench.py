"""Measures the raw-frame route (csrc/frames.hip scl_frames_debayer, DeviceResizer.debayer) on the
MI355X: 960 x 1280 'gbrg' Bayer frames with a lens-like distortion table, in one process on one box.
Every route is warmed before it is timed; raw frames, the table and the resize tables are resident and
the outputs preallocated.

(a) per call, at 1 and at 25 frames ("queued": HIP events around a back-to-back run of calls that fills
    at least 0.2 s; "kernels": the sum over the route's launches of the median of HIP events around each
    single launch, scl_prof_begin / _end — own kernels only, so the torch composition has none):
      full        scl_frames_debayer at full size, uint8 [n,960,1280,3]
      full+resize that, then scl_frames_resize to float32 [n,180,240,3]          (two launches)
      fused       scl_frames_debayer with resize_img(240)'s tables, float32     (one launch)
      torch       the same mathematics composed from torch operators on the device: conv2d (float32) on
                  the three masked planes, a gather at indices and with weights prepared once from the
                  table, the byte, then scl_frames_resize.  It need not be bit-equal; the number of
                  differing values is printed.
    and the bytes each own launch needs, counted from its shapes (device_cv.debayer_bytes).
(b) the host statement (robotcar.load_image_np + cv.apply_plan), one thread, per frame.
(c) one raw frame per call, synchronised, against an index of 100 000 x 256:
    Localizer.locate_raw(bayer='gbrg', lut=...) against locate_raw of the same frame already demosaiced
    (the route of profiles/device_resize) and against the host statement + locate.

The claims under test, stated before measuring:
  1. the fused route is faster than full size + scl_frames_resize, at 1 and at 25 frames;
  2. both are faster than the torch composition, at 1 and at 25 frames.

    python scripts/robotcar_raw_bench.py [--out profiles/robotcar_raw/robotcar_raw_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import device_resize_bench as B  # noqa: E402  (median, queued_us, wall_ms)
from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.util import cv, device_cv, robotcar  # noqa: E402

SH, SW, PATTERN, BORDER = 960, 1280, 'gbrg', 'reflect'
OWN = ('frames_debayer_kernel', 'frames_resize_kernel')


def lens_lut(sh, sw, seed=1):
    """Scale 0.9 about the centre, an offset, noise below 1 px."""
    rng = np.random.default_rng(seed)
    ident = robotcar.identity_lut(sh, sw)
    cx, cy = (sw - 1) / 2.0, (sh - 1) / 2.0
    return np.stack([cx + 0.9 * (ident[0] - cx) + 3.25 + rng.uniform(-0.9, 0.9, sh * sw),
                     cy + 0.9 * (ident[1] - cy) - 2.5 + rng.uniform(-0.9, 0.9, sh * sw)])


def kernels_us(fn, launches=100):
    """Sum over the own kernels of the median duration of one launch."""
    with L.KernelTimer(4 * launches) as kt:
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
    return sum(B.median([ms for name, ms in kt.records if name == k]) * 1e3
               for k in OWN if any(name == k for name, _ in kt.records))


class TorchRoute:
    """conv2d on the masked planes, gather, weights, byte — prepared once per (table, pattern)."""

    def __init__(self, lut, dev):
        sh, sw = SH, SW
        self.masks = torch.from_numpy(robotcar.masks(sh, sw, PATTERN).astype(np.float32)).to(dev)
        k = np.stack([[[1, 2, 1], [2, 4, 2], [1, 2, 1]], [[0, 1, 0], [1, 4, 1], [0, 1, 0]],
                      [[1, 2, 1], [2, 4, 2], [1, 2, 1]]]).astype(np.float32) / 4
        self.kern = torch.from_numpy(k[:, None]).to(dev)
        lx, ly = lut[0], lut[1]
        inside = (ly >= 0) & (ly <= sh - 1) & (lx >= 0) & (lx <= sw - 1)
        ly, lx = np.where(inside, ly, 0.0), np.where(inside, lx, 0.0)
        y0, x0 = np.floor(ly).astype(np.int64), np.floor(lx).astype(np.int64)
        ty, tx = ly - y0, lx - x0
        y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
        self.idx = [torch.from_numpy(a * sw + b).to(dev) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
        self.w = [torch.from_numpy((a * b * inside).astype(np.float32)).to(dev)
                  for a, b in ((1 - ty, 1 - tx), (1 - ty, tx), (ty, 1 - tx), (ty, tx))]

    def full(self, raw):
        n = raw.shape[0]
        planes = raw.float()[:, None] * self.masks[None]
        v = F.conv2d(F.pad(planes, (1, 1, 1, 1), mode='replicate'), self.kern, groups=3).reshape(n, 3, -1)
        acc = v[..., self.idx[0]] * self.w[0]
        for i, w in zip(self.idx[1:], self.w[1:]):
            acc = acc + v[..., i] * w
        return acc.to(torch.int32).to(torch.uint8).view(n, 3, SH, SW).permute(0, 2, 3, 1).contiguous()


def kernel_section(dev, lines):
    rng = np.random.default_rng(3)
    lut_host = lens_lut(SH, SW)
    lut = torch.from_numpy(lut_host).to(dev)
    plan = cv.plan_resize_img(SH, SW, 240)
    xtab, ytab = torch.from_numpy(plan.xtab()).to(dev), torch.from_numpy(plan.ytab()).to(dev)
    torch_route = TorchRoute(lut_host, dev)
    host_raw = rng.integers(0, 256, size=(25, SH, SW), dtype=np.uint8)
    t, want0 = [], None
    for k in range(3):                                    # (b) the host statement, per frame
        t0 = time.perf_counter()
        got = cv.apply_plan(robotcar.load_image_np(host_raw[0], PATTERN, lut_host, BORDER), plan)
        t.append(time.perf_counter() - t0)
        want0 = got
    host_ms = B.median(t) * 1e3
    lines.append('(a) per call: raw frames %d x %d %s, table and resize tables resident; resize_img(240) -> %d x %d'
                 % (SH, SW, PATTERN, plan.dh, plan.dw))
    verdict = {}
    for n in (1, 25):
        raw = torch.from_numpy(host_raw[:n]).to(dev)
        full = torch.empty((n, SH, SW, 3), dtype=torch.uint8, device=dev)
        small = torch.empty((n, plan.dh, plan.dw, 3), dtype=torch.float32, device=dev)
        small2, small3 = torch.empty_like(small), torch.empty_like(small)

        def r_full():
            device_cv.debayer_tables(raw, PATTERN, BORDER, lut, None, None, full)

        def r_two():
            device_cv.debayer_tables(raw, PATTERN, BORDER, lut, None, None, full)
            device_cv.apply_tables(full, xtab, ytab, small2)

        def r_fused():
            device_cv.debayer_tables(raw, PATTERN, BORDER, lut, xtab, ytab, small)

        def r_torch():
            device_cv.apply_tables(torch_route.full(raw), xtab, ytab, small3)
        for fn in (r_two, r_fused, r_torch):
            fn()
        torch.cuda.synchronize()
        same = torch.equal(small, small2) and np.array_equal(small[0].cpu().numpy(), want0.astype(np.float32))
        differ = int((small3 != small).sum())
        nb_full = device_cv.debayer_bytes(n, SH, SW, SH, SW, 1, True, False)
        nb_fused = device_cv.debayer_bytes(n, SH, SW, plan.dh, plan.dw, 4, True, True)
        nb_resize = device_cv.kernel_bytes(n, plan.dh, plan.dw, 3, 4)
        rows = [('full', r_full, nb_full), ('full+resize', r_two, nb_full + nb_resize), ('fused', r_fused, nb_fused),
                ('torch', r_torch, None)]
        q = {}
        for name, fn, nbytes in rows:
            q[name], iters = B.queued_us(fn)
            if nbytes is None:
                lines.append('  n = %2d  %-12s queued %9.2f us/call (%6d calls)   %d of %d values differ from the kernel\'s'
                             % (n, name, q[name], iters, differ, small.numel()))
                continue
            k_us = kernels_us(fn)
            lines.append('  n = %2d  %-12s queued %9.2f us/call (%6d calls)   kernels %9.2f us   %8.3f MB needed -> %7.1f GB/s'
                         % (n, name, q[name], iters, k_us, nbytes / 1e6, nbytes / k_us / 1e3))
        lines.append('  n = %2d  fused == full+resize == host statement (frame 0): %s'
                     % (n, 'bit-equal' if same else 'RESULTS DIFFER'))
        verdict[n] = (q['fused'] < q['full+resize'], q['fused'] < q['torch'] and q['full+resize'] < q['torch'], q)
    lines.append('(b) host statement, robotcar.load_image_np + cv.apply_plan, one thread: %.1f ms/frame (median of 3)' % host_ms)
    for n, (c1, c2, q) in verdict.items():
        lines.append('claim 1 at n = %2d "fused is faster than full size + scl_frames_resize": %s (%.2f us against %.2f us)'
                     % (n, 'HOLDS' if c1 else 'DOES NOT HOLD', q['fused'], q['full+resize']))
        lines.append('claim 2 at n = %2d "both are faster than the torch composition": %s (%.2f us and %.2f us against %.2f us)'
                     % (n, 'HOLDS' if c2 else 'DOES NOT HOLD', q['fused'], q['full+resize'], q['torch']))
    return host_raw[0], lut_host


def locate_section(dev, raw, lut, lines):
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.model import nets, reduction
    model = nets.VGG16NetVLAD().to(dev).eval()
    reduction.attach(model, '1fc', B.D, height=180, width=240)
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((B.R, B.D), dtype=np.float32)
    loc = localize.Localizer(ref, np.stack([0.5 * np.arange(B.R), np.zeros(B.R)], 1), model=model, n=B.N, device=dev)
    rgb = robotcar.load_image_np(raw, PATTERN, lut, BORDER)

    def raw_route():
        return loc.locate_raw(raw, bayer=PATTERN, lut=lut, border=BORDER)

    def rgb_route():
        return loc.locate_raw(rgb)
    same = torch.equal(loc.prepare_raw(raw, bayer=PATTERN, lut=lut, border=BORDER), loc.prepare_raw(rgb))
    hits = np.array_equal(raw_route()[0], rgb_route()[0])
    (t_raw, t_rgb), reps = B.wall_ms([raw_route, rgb_route])
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loc.locate(cv.resize_img(robotcar.load_image_np(raw, PATTERN, lut, BORDER), 240)[None].astype(np.float32))
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    lines.append('(c) one raw %d x %d frame per call (pageable NumPy), synchronised, index %d x %d, n = %d; medians of %d '
                 'calls, the two device routes in turn' % (SH, SW, B.R, B.D, B.N, reps))
    lines.append('  locate_raw(bayer=..., lut=...)   raw mosaic, 1.2 MB up         %8.3f ms/frame' % t_raw)
    lines.append('  locate_raw                        demosaiced frame, 3.7 MB up  %8.3f ms/frame' % t_rgb)
    lines.append('  host statement + resize + locate (median of 3)                 %8.3f ms/frame' % (B.median(t) * 1e3))
    lines.append('  network input of the raw route: %s; references named: %s'
                 % ('bit-equal to the demosaiced route\'s' if same else 'RESULTS DIFFER', 'the same' if hits else 'OTHERS'))
    return same and hits


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'robotcar_raw_bench.py measures on a HIP device'
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs; torch %s, HIP %s; one run, every route warmed first'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                torch.__version__, torch.version.hip)]
    raw, lut = kernel_section(dev, lines)
    ok = locate_section(dev, raw, lut, lines)
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    return 0 if ok and 'RESULTS DIFFER' not in text else 1


if __name__ == '__main__':
    sys.exit(main())

"""Measures the device resize (csrc/frames.hip scl_frames_resize, util/device_cv.py) on the MI355X
against the host resampler it reproduces (util/cv.py), in one process on one box.  Every shape is
warmed before it is timed.

(a) The kernel alone, source and tables resident, both output kinds, at
      1 x 960 x 1280 x 3 -> 180 x 240 (resize_img 240), 25 x the same, and
      24 x 480 x 640 x 3 -> standard_size(180, 240):
    * "queued": HIP events around a run of back-to-back calls that fills at least 0.2 s, per call
      (at one frame this is the rate at which the host can enqueue: the grid is ~170 workgroups);
    * "kernel": the median of HIP events around each single launch (scl_prof_begin / _end);
    * the bytes the launch needs, counted from its shapes (device_cv.kernel_bytes: 2 x 2 source
      bytes in and one value out per output value, the tables), over the kernel time.
(b) ``cv.resize_img`` on the host for the same frames, on one thread, per frame.
(c) One frame at a time, synchronised, against an index of 100 000 x 256 (the network carries a
    256-wide dense head, the references are random): wall time per frame of
      host route     cv.resize_img + Localizer.locate of the float32 frame,
      locate_raw     of a pageable NumPy frame (through the resizer's pinned staging buffer),
      locate_raw     of a pinned host tensor,
    the three taken in turn, medians; and the split of the device route into upload, resize,
    network (the backbone and head at one frame) and retrieval, each stage synchronised.

The claim under test: locate_raw takes less wall time per frame than the host resize + locate of
the same run.  The verdict is printed; the feature is bit-equal either way.

    python scripts/device_resize_bench.py [--out profiles/device_resize/device_resize_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.util import cv, device_cv  # noqa: E402

FILL_S = 0.2
R, D, N = 100000, 256, 5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def queued_us(fn, fill_s=FILL_S):
    """Per call, from HIP events around a back-to-back run of calls that lasts at least fill_s."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    iters, total = 50, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        total = a.elapsed_time(b) * 1e-3
        if total >= fill_s:
            return total / iters * 1e6, iters
        iters = int(iters * max(2.0, 1.2 * fill_s / max(total, 1e-6))) + 1


def kernel_us(fn, launches=200):
    with L.KernelTimer(launches) as kt:
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
    return median(ms for name, ms in kt.records if name == 'frames_resize_kernel') * 1e3


def wall_ms(fns, fill_s=FILL_S, warmup=5, reps=None):
    """Medians (ms) of synchronised calls taken in turn f0, f1, ..: ``reps`` rounds, or until every
    function has run for fill_s (and 20 rounds)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    while len(times[0]) < reps if reps else (min(sum(t) for t in times) < fill_s or len(times[0]) < 20):
        for t, fn in zip(times, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
    return [median(t) * 1e3 for t in times], len(times[0])


def kernel_section(dev, lines):
    rng = np.random.default_rng(3)
    shapes = [('1 x 960x1280x3 -> 180x240  resize_img(240)', (1, 960, 1280, 3), cv.plan_resize_img(960, 1280, 240)),
              ('25 x 960x1280x3 -> 180x240 resize_img(240)', (25, 960, 1280, 3), cv.plan_resize_img(960, 1280, 240)),
              ('24 x 480x640x3 -> 180x240  standard_size', (24, 480, 640, 3), cv.plan_standard_size(480, 640, 180, 240))]
    frames = {}
    lines.append('(a) kernel alone (source and tables resident); (b) cv.resize_img / standard_size on one host thread')
    for label, shape, plan in shapes:
        host = rng.integers(0, 256, size=shape, dtype=np.uint8)
        frames[shape] = host
        src = torch.from_numpy(host).to(dev)
        xtab, ytab = torch.from_numpy(plan.xtab()).to(dev), torch.from_numpy(plan.ytab()).to(dev)
        n, c = shape[0], shape[3]
        want = np.stack([cv.apply_plan(f, plan) for f in host[:2]])
        for out in (torch.uint8, torch.float32):
            dst = torch.empty((n, plan.dh, plan.dw, c), dtype=out, device=dev)

            def call():
                device_cv.apply_tables(src, xtab, ytab, dst)
            call()
            same = np.array_equal(dst[:2].cpu().numpy(), want.astype(np.float32 if out == torch.float32 else np.uint8))
            q_us, iters = queued_us(call)
            k_us = kernel_us(call)
            nbytes = device_cv.kernel_bytes(n, plan.dh, plan.dw, c, dst.element_size())
            lines.append('  %-44s out %-7s queued %8.2f us/call (%6d calls)   kernel %8.2f us   %7.3f MB needed -> '
                         '%6.1f GB/s   %s' % (label, str(out).replace('torch.', ''), q_us, iters, k_us, nbytes / 1e6,
                                              nbytes / k_us / 1e3, 'bit-equal' if same else 'RESULTS DIFFER'))
        # (b) the host resampler, per frame, one thread
        take = host[:min(n, 6)]
        for f in take[:2]:
            cv.apply_plan(f, plan)                      # warm
        t, reps = [], 0
        while sum(t) < FILL_S:
            f = take[reps % len(take)]
            t0 = time.perf_counter()
            cv.resize_img(f, 240) if 'resize_img' in label else cv.standard_size(f, 180, 240)
            t.append(time.perf_counter() - t0)
            reps += 1
        lines.append('  %-44s host, one thread: %8.3f ms/frame (median of %d; %.1f ms for the %d frames)'
                     % ('', median(t) * 1e3, reps, median(t) * 1e3 * n, n))
    return frames[(1, 960, 1280, 3)][0]


def locate_section(dev, frame, lines):
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.model import nets, reduction
    model = nets.VGG16NetVLAD().to(dev).eval()
    reduction.attach(model, '1fc', D, height=180, width=240)
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((R, D), dtype=np.float32)
    ref_xy = np.stack([0.5 * np.arange(R), np.zeros(R)], 1)
    loc = localize.Localizer(ref, ref_xy, model=model, n=N, device=dev)
    pinned = torch.from_numpy(frame).pin_memory()

    def host_route():
        return loc.locate(cv.resize_img(frame, 240)[None].astype(np.float32))

    def raw_pageable():
        return loc.locate_raw(frame)

    def raw_pinned():
        return loc.locate_raw(pinned)
    same = torch.equal(loc.prepare_raw(frame).cpu()[0], torch.from_numpy(cv.resize_img(frame, 240).astype(np.float32)))
    hits = np.array_equal(host_route()[0], raw_pageable()[0]) and np.array_equal(host_route()[0], raw_pinned()[0])
    (t_host, t_page, t_pin), reps = wall_ms([host_route, raw_pageable, raw_pinned])
    lines.append('(c) one 960x1280x3 frame per call, synchronised, index %d x %d, n = %d; medians of %d calls, '
                 'the three routes in turn' % (R, D, N, reps))
    lines.append('  host route  cv.resize_img + locate        %8.3f ms/frame' % t_host)
    lines.append('  locate_raw  pageable NumPy frame          %8.3f ms/frame   (%.3f x the host route)'
                 % (t_page, t_page / t_host))
    lines.append('  locate_raw  pinned host tensor            %8.3f ms/frame   (%.3f x the host route)'
                 % (t_pin, t_pin / t_host))
    lines.append('  network input of the device route: %s; references named: %s'
                 % ('bit-equal to the host route\'s' if same else 'RESULTS DIFFER', 'the same' if hits else 'OTHERS'))

    # the split: every stage synchronised on its own
    resizer = loc._resizer
    state = {}

    def host_resize():
        state['host'] = cv.resize_img(frame, 240)[None].astype(np.float32)

    def host_upload():
        state['host_dev'] = torch.from_numpy(state['host']).to(dev)

    def upload_pageable():
        state['src'] = resizer._upload(frame[None])

    def upload_pinned():
        state['src'] = resizer._upload(pinned[None])

    xtab, ytab = resizer._device_tables((960, 1280, 'resize_img', 240), None)
    dst = torch.empty((1, 180, 240, 3), dtype=torch.float32, device=dev)

    def resize():
        state['x'] = device_cv.apply_tables(state['src'], xtab, ytab, dst)

    def network():
        with torch.no_grad():
            state['desc'] = nets.output(state['x'], model=model).float()

    def retrieve():
        state['hit'] = loc.locate_descriptors(state['desc'])
    stages = [('host: cv.resize_img + float32', host_resize), ('host: float32 upload (518 KB, pageable)', host_upload),
              ('device: uint8 upload (3.7 MB, pageable via staging)', upload_pageable),
              ('device: uint8 upload (3.7 MB, pinned source)', upload_pinned),
              ('device: resize kernel (float32 out)', resize), ('network: backbone + head, one frame', network),
              ('retrieval: whitening-free index query + read-back', retrieve)]
    ts, reps = wall_ms([fn for _, fn in stages], reps=60)
    lines.append('  split, each stage synchronised (medians of %d):' % reps)
    for (label, _), t in zip(stages, ts):
        lines.append('    %-52s %8.3f ms' % (label, t))
    won = t_page < t_host
    lines.append('claim "locate_raw takes less wall time per frame than the host resize + locate": %s '
                 '(pageable %.3f ms, pinned %.3f ms against %.3f ms)' % ('HOLDS' if won else 'DOES NOT HOLD',
                                                                         t_page, t_pin, t_host))
    return same


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'device_resize_bench.py measures on a HIP device'
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs; torch %s, HIP %s; one run, every shape warmed first'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                torch.__version__, torch.version.hip)]
    frame = kernel_section(dev, lines)
    ok = locate_section(dev, frame, lines)
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    return 0 if ok and 'RESULTS DIFFER' not in text else 1


if __name__ == '__main__':
    sys.exit(main())

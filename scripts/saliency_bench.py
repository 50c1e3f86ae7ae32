"""Match saliency: the HIP kernels (csrc/saliency.hip) against a plain torch composition of the same
mathematics, and the whole explain + overlay call either way.

  python scripts/saliency_bench.py --out profiles/saliency/saliency_bench.txt

Shapes: B = 1 and B = 25 frames, 180 x 240 (the reference's training resolution: an 11 x 15 map) and
480 x 640 (30 x 40).  Per shape, in ONE process:
  * map      scl_saliency_map  | mean / einsum / relu / amax                         (per mode, per dtype)
  * overlay  scl_saliency_overlay | F.interpolate(bilinear, align_corners=False), LUT gather, blend
  * explain  MatchSaliency.explain + overlay | the same forward and head backward, then the torch
             composition of map and overlay (bf16 model, Grad-CAM)
Device events around `--iters` calls, after a warm-up of every shape; the two sides alternate within a
round, `--rounds` rounds; the median round is reported with the fastest and the slowest.  The torch
composition's map is compared with the kernel's at every shape (printed: a faster, different result
would not be faster).  Needs a HIP device: there is no CPU timing path.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd.evaluation import saliency  # noqa: E402
from soft_contrastive_learning_amd.model import nets  # noqa: E402

SHAPES = [(1, 180, 240), (25, 180, 240), (1, 480, 640), (25, 480, 640)]       # (B, H, W): map H/16 x W/16


def torch_map(act, grad, mode):
    g = grad.float()
    if mode == 'gradnorm':
        m = (g * g).sum(-1).sqrt()
    else:
        m = torch.relu(torch.einsum('bc,bhwc->bhw', g.mean((1, 2)), act.float()))
    return m, m.amax((1, 2))


def torch_overlay(frames, m, scale, lut, alpha):
    up = F.interpolate(m[:, None], size=frames.shape[1:3], mode='bilinear', align_corners=False)[:, 0]
    s = scale[:, None, None]
    r = torch.where(s > 0, up / s, torch.zeros_like(up)).nan_to_num(0.0).clamp(0.0, 1.0)
    colour = lut[(r * 255.0 + 0.5).long()]
    return ((alpha * colour + (256 - alpha) * frames.int() + 128) >> 8).to(torch.uint8)


def time_pair(fns, iters, rounds, warmup):
    """[median, min, max] microseconds per call for each of ``fns``, alternating within a round."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(1000.0 * e0.elapsed_time(e1) / iters)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--out', default='')
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--explain_iters', type=int, default=5)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--warmup', type=int, default=5)
    flags = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('saliency_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say('# microseconds per call: median of %d rounds [fastest .. slowest], %d calls per round (explain: %d)'
        % (flags.rounds, flags.iters, flags.explain_iters))
    say('%-34s %-28s %-28s %s' % ('case', 'HIP', 'torch', 'torch / HIP'))
    lut_u8 = torch.from_numpy(saliency.default_lut()).to(dev)
    lut_i32 = lut_u8.int()
    model = nets.VGG16NetVLAD(compute_dtype=torch.bfloat16).to(dev).eval()
    sal = saliency.MatchSaliency(model)
    verdict = {}
    gen = torch.Generator().manual_seed(0)

    def row(name, shape, res):
        (hm, hlo, hhi), (tm, tlo, thi) = res
        say('%-34s %9.1f [%7.1f ..%8.1f] %9.1f [%7.1f ..%8.1f] %8.2f'
            % (name, hm, hlo, hhi, tm, tlo, thi, tm / hm))
        verdict.setdefault(shape, []).append((name, tm / hm))

    for b, H, W in SHAPES:
        h, w = H // 16, W // 16
        shape = 'B=%d %dx%d->%dx%d' % (b, h, w, H, W)
        frames = torch.randint(0, 256, (b, H, W, 3), generator=gen, dtype=torch.uint8).to(dev)
        for dtype, tag in ((torch.bfloat16, 'bf16'), (torch.float32, 'f32')):
            act = torch.randn(b, h, w, 512, generator=gen).to(dev, dtype)
            grad = torch.randn(b, h, w, 512, generator=gen).to(dev, dtype)
            for mode in ('gradcam', 'gradnorm'):
                got, _ = saliency.saliency_map(act, grad, mode)
                want, _ = torch_map(act, grad, mode)
                err = float((got - want).abs().max() / want.abs().max())
                res = time_pair([lambda: saliency.saliency_map(act, grad, mode), lambda: torch_map(act, grad, mode)],
                                flags.iters, flags.rounds, flags.warmup)
                row('map %s %s %s' % (mode, tag, shape), shape, res)
                say('#   max |HIP - torch| / max |torch| = %.2e' % err)
        m, scale = saliency.saliency_map(act, grad, 'gradcam')
        same = float((saliency.overlay(frames, m, scale).int() - torch_overlay(frames, m, scale, lut_i32, 128).int()).abs().max())
        res = time_pair([lambda: saliency.overlay(frames, m, scale), lambda: torch_overlay(frames, m, scale, lut_i32, 128)],
                        flags.iters, flags.rounds, flags.warmup)
        row('overlay %s' % shape, shape, res)
        say('#   max |HIP - torch| over the pixels = %d of 255' % same)
        images = frames.float()
        target = sal.embed(torch.randint(0, 256, (b, H, W, 3), generator=gen).float().to(dev))

        def hip_whole():
            mm, ss = sal.explain(images, target)
            return saliency.overlay(frames, mm, ss)

        def torch_whole():
            a, g, _ = sal.map_gradient(images, target)
            mm, ss = torch_map(a, g, 'gradcam')
            return torch_overlay(frames, mm, ss, lut_i32, 128)

        res = time_pair([hip_whole, torch_whole], flags.explain_iters, flags.rounds, 2)
        row('explain+overlay bf16 %s' % shape, shape, res)
    say('')
    say('# the claim: the HIP route is the faster one at each of the four shapes')
    for shape, rows in verdict.items():
        lost = [name for name, ratio in rows if ratio < 1.0]
        say('# %-28s %s' % (shape, 'held in every row' if not lost else 'did NOT hold for: ' + '; '.join(lost)))
    if flags.out:
        os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
        with open(flags.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

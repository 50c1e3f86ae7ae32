"""The NetVLAD head from data: one Lloyd iteration on the HIP kernels (csrc/kmeans.hip) against a plain
torch composition of the same mathematics, k-means as a whole, and init_head as a whole.

  python scripts/vlad_init_bench.py --out profiles/vlad_init/vlad_init_bench.txt

In ONE process:
  * iteration  offsets + scl_kmeans_assign + scl_kmeans_update | x @ c.T - off, argmax, index_add_,
               bincount, division, the inertia                  (N = 50 000, K = 64, D = 512)
  * kmeans     vlad_init.kmeans(iters=100) on the same rows: iterations run, milliseconds
  * init_head  500 synthetic 180 x 240 frames, 100 descriptors each, bf16 backbone: milliseconds, of which
               the frames' synthesis and upload, the backbone passes and the clustering
Device events around `--iters` calls after a warm-up; the two sides alternate within a round, `--rounds`
rounds; the median round is reported with the fastest and the slowest.  The torch composition's labels
are compared with the kernel's (printed: a faster, different result would not be faster).  The claim,
stated before the run: the HIP iteration is the faster one.  Needs a HIP device.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd.model import nets, vlad_init  # noqa: E402
from soft_contrastive_learning_amd.train import dataset  # noqa: E402


def torch_iteration(x, c, xsq):
    off = 0.5 * (c.double() ** 2).sum(1).float()
    score = x @ c.t() - off
    best, label = score.max(dim=1)
    sums = torch.zeros_like(c).index_add_(0, label, x)
    counts = torch.bincount(label, minlength=c.shape[0])
    new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None].float(), c)
    return new, label, (xsq - 2.0 * best.double()).sum()


def hip_iteration(x, c):
    got = vlad_init.assign(x, c, vlad_init.device_offsets(c), sums=True)
    new, counts, inertia = vlad_init.update(got['part_sum'], got['part_cnt'], got['part_inertia'], c)
    return new, got['label'], inertia


def time_pair(fns, iters, rounds, warmup):
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
    p.add_argument('--n', type=int, default=50000)
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--frames', type=int, default=500)
    flags = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('vlad_init_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say('# the claim, before the run: the HIP iteration is the faster one')
    rng = np.random.RandomState(0)
    m = rng.randn(64, 512)
    xh = m[rng.randint(0, 64, flags.n)] + 1.5 * rng.randn(flags.n, 512)
    x = torch.from_numpy((xh / np.sqrt((xh * xh).sum(1, keepdims=True))).astype(np.float32)).to(dev)
    c = x[torch.from_numpy(np.random.RandomState(0).permutation(flags.n)[:64]).to(dev)].contiguous()
    xsq = (x.double() ** 2).sum(1)
    hn, hl, hi = hip_iteration(x, c)
    tn, tl, ti = torch_iteration(x, c, xsq)
    say('# N = %d, K = 64: labels that differ %d, max |centre difference| %.2e, inertia %.6f | %.6f'
        % (flags.n, int((hl.long() != tl).sum()), float((hn - tn).abs().max()), float(hi), float(ti)))
    (hm, hlo, hhi), (tm, tlo, thi) = time_pair([lambda: hip_iteration(x, c), lambda: torch_iteration(x, c, xsq)],
                                               flags.iters, flags.rounds, flags.warmup)
    say('# microseconds per Lloyd iteration: median of %d rounds [fastest .. slowest], %d calls per round'
        % (flags.rounds, flags.iters))
    say('%-12s %9.1f [%7.1f ..%8.1f]' % ('HIP', hm, hlo, hhi))
    say('%-12s %9.1f [%7.1f ..%8.1f]' % ('torch', tm, tlo, thi))
    say('# torch / HIP = %.2f: the claim %s' % (tm / hm, 'HELD' if tm > hm else 'did NOT hold'))

    vlad_init.kmeans(x, 64, iters=2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = vlad_init.kmeans(x, 64, iters=100)
    torch.cuda.synchronize()
    whole = time.perf_counter() - t0
    say('kmeans(iters=100): %d iterations to fixed labels, %.1f ms, inertia %.3f -> %.3f, empty clusters %d'
        % (res.iterations, 1e3 * whole, res.inertia[0], res.inertia[-1], res.empty))

    model = nets.VGG16NetVLAD(compute_dtype=torch.bfloat16).to(dev).eval()
    frames = dataset.SyntheticImageSet(flags.frames, 180, 240, seed=0)
    idx = np.arange(flags.frames)
    vlad_init.init_head(model, frames, idx[:24], 24, per_image=100, iters=5)           # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [frames.load_images(idx[s:s + 24]) for s in range(0, flags.frames, 24)]
    t_host = time.perf_counter() - t0

    class Ready:                       # the frames already synthesised: what is left is upload + backbone
        def load_images(self, indices):
            return host[int(indices[0]) // 24]

    t0 = time.perf_counter()
    xs = vlad_init.sample_descriptors(model, Ready(), idx, 24, per_image=100, seed=0)
    torch.cuda.synchronize()
    t_backbone = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = vlad_init.kmeans(xs, 64, iters=100)
    vlad_init.head_from_centres(res.centres, xs)
    torch.cuda.synchronize()
    t_cluster = time.perf_counter() - t0
    t0 = time.perf_counter()
    rec = vlad_init.init_head(model, frames, idx, 24, per_image=100, iters=100)
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    say('init_head on %d synthetic 180 x 240 frames (N = %d): %.0f ms as a whole; apart: synthesis on the host '
        '%.0f ms, upload + backbone %.0f ms, k-means (%d iterations) + head %.0f ms; alpha %.2f'
        % (flags.frames, rec['N'], 1e3 * t_all, 1e3 * t_host, 1e3 * t_backbone, rec['iterations'],
           1e3 * t_cluster, rec['alpha']))
    if flags.out:
        os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
        with open(flags.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

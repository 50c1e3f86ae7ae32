"""Measures the HIP parameter update (train/optim.py HipAdam, csrc/optim.hip) on the MI355X against
what it can replace, in one process on one box.

Builds ``VGG16NetVLAD`` and ``GradBuckets`` as bench.py does (14.8 M float32 parameters, every
``.grad`` a view into one flat buffer) — twice, one model per optimizer — fills the flat buffers
with random gradients and times, with HIP events around each call, medians of --reps calls after a
warm-up:

* ``TFAdam(fused=True).step()`` — torch's multi-tensor kernels, the yardstick of THIS run;
* ``HipAdam.step()`` — one scl_apply_adam launch;
* ``scl_grad_stats`` over the flat buffer (the pass --skip_nonfinite adds in front of the update).

An Adam update reads var, m, v and g and writes var, m, v: 28 bytes per element; the achieved
bytes/s of both optimizers are printed against that, and the 4 bytes per element of the statistics
pass.  The expectation stated and checked (exit status 1 when missed): HipAdam is no slower than
1.05 x TFAdam(fused=True) of the same run.

    python scripts/optimizer_bench.py [--reps 50] [--out profiles/optimizer/optimizer_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import parallel  # noqa: E402
from soft_contrastive_learning_amd.model import nets  # noqa: E402
from soft_contrastive_learning_amd.train.optim import GradStats, HipAdam, TFAdam  # noqa: E402

MARGIN = 1.05      # the run-to-run and box-to-box spread this project reports is +- 4 %


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def event_us(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median(a.elapsed_time(b) * 1e3 for a, b in ev)


def setup(dev, seed):
    model = nets.VGG16NetVLAD(compute_dtype=torch.float32, seed=1234).to(dev)
    params = nets.trainable_parameters(model)
    buckets = parallel.GradBuckets(params)
    gen = torch.Generator(device=dev).manual_seed(seed)
    buckets.flat.copy_(torch.randn(buckets.flat.numel(), generator=gen, device=dev) * 1e-4)
    return params, buckets


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'optimizer_bench.py measures on a HIP device'
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs, %.0f GB; torch %s, HIP %s'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                prop.total_memory / 1e9, torch.__version__, torch.version.hip)]
    params_t, buckets_t = setup(dev, 1)
    params_h, buckets_h = setup(dev, 1)
    n = buckets_h.flat.numel()
    old = TFAdam(params_t, lr=5e-6, fused=True)
    new = HipAdam(params_h, lr=5e-6)
    stats = GradStats(buckets_h.flat)
    # in turn, twice: the second round of each is the one reported (the first also warms the other's caches)
    t = {}
    for _ in range(2):
        t['TFAdam(fused=True).step()'] = (event_us(old.step, f.reps), 28)
        t['HipAdam.step()'] = (event_us(new.step, f.reps), 28)
        t['scl_grad_stats'] = (event_us(stats.run, f.reps), 4)
    lines.append('%d float32 parameters in %d tensors, gradients in one flat buffer; medians of %d calls, HIP '
                 'events around each call' % (n, len(params_h), f.reps))
    for name, (us, per) in t.items():
        lines.append('%-28s %8.1f us   %2d bytes per element   %6.2f TB/s' % (name, us, per, per * n / us / 1e6))
    ratio = t['HipAdam.step()'][0] / t['TFAdam(fused=True).step()'][0]
    ok = ratio <= MARGIN
    lines.append('HipAdam / TFAdam(fused=True) = %.3f (expected <= %.2f): %s'
                 % (ratio, MARGIN, 'met' if ok else 'MISSED'))
    ss, bad = stats.read()
    lines.append('grad_stats of the flat buffer: norm %.6g, %d non-finite; HipAdam after %d steps: powers %r'
                 % (ss ** 0.5, bad, new.beta_powers()[2], new.beta_powers()[:2]))
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    nets.GRAD_SINK = None
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

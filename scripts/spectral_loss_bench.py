"""Times the wrd / prodwrd / sumwrd losses (csrc/spectral_loss.hip) on the MI355X.

At the trainer's shape (T = 2, P = N = 12, E = 32768 by default): forward and backward of each
loss in microseconds (median of --reps calls, HIP events around each, allocations and the Python
of the autograd Function included), the kernels of one forward + backward with their own
durations (KernelTimer), and next to them the same loss written with torch.linalg.svdvals and
autograd in float32 on the same device — what a caller had before these kernels.  One JSON line
per loss with --json.

    python scripts/spectral_loss_bench.py [--tuples 2] [--positives 12] [--negatives 12]
                                          [--width 32768] [--dimensions 10] [--reps 20] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.model import losses as M  # noqa: E402
from tests import spectral_data as D  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2]


def svdvals_loss(kind, a, pos, neg, pw, nw, margin, k, ap=2.0, an=50.0, lamb=1.0):
    """model/losses.py:373-437 on torch ops."""
    others = torch.cat([pos, neg], 1)
    res = others - a
    if kind == 'wrd':
        yp, yn = res * pw, res * nw
    else:
        sim = a @ others.transpose(1, 2)
        fp = (1.0 / (1.0 + torch.exp(ap * (sim - lamb)))).transpose(1, 2)
        fn = (1.0 / (1.0 + torch.exp(an * (lamb - sim)))).transpose(1, 2)
        yp, yn = (res * pw * fp, res * nw * fn) if kind == 'prodwrd' else (res * (pw + fp), res * (nw + fn))
    sp = torch.linalg.svdvals(yp)[:, :k]
    sn = torch.linalg.svdvals(yn)[:, :k]
    return (sp.prod(1) - sn.prod(1) + margin).mean(0)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--tuples', type=int, default=2)
    p.add_argument('--positives', type=int, default=12)
    p.add_argument('--negatives', type=int, default=12)
    p.add_argument('--width', type=int, default=32768)
    p.add_argument('--dimensions', type=int, default=10)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--json', action='store_true')
    f = p.parse_args(argv)
    dev = torch.device('cuda:0')
    t, np_, nn, e, k = f.tuples, f.positives, f.negatives, f.width, f.dimensions
    z, pw, nw = D.tuples(t, np_, nn, e, seed=5)
    zt = torch.tensor(z, device=dev)
    a = zt[:, :1].clone().requires_grad_(True)
    pos = zt[:, 1:1 + np_].clone().requires_grad_(True)
    neg = zt[:, 1 + np_:].clone().requires_grad_(True)
    pwt, nwt = torch.tensor(pw, device=dev)[:, :, None], torch.tensor(nw, device=dev)[:, :, None]
    print('T=%d P=%d N=%d E=%d dimensions=%d: input %.1f MB' % (t, np_, nn, e, k, zt.numel() * 4 / 1e6))
    out = []
    for kind in ('wrd', 'prodwrd', 'sumwrd'):
        fn = getattr(M, kind + '_loss')

        def ours():
            return fn(a, pos, neg, pwt, nwt, 0.1, dimensions=k)

        def theirs():
            return svdvals_loss(kind, a, pos, neg, pwt, nwt, 0.1, k)

        def fwd_bwd(make):
            def go():
                for x in (a, pos, neg):
                    x.grad = None
                make().backward()
            return go
        with torch.no_grad():
            t_f = timed(ours, f.reps)
            t_fr = timed(theirs, f.reps)
        t_fb = timed(fwd_bwd(ours), f.reps)
        t_fbr = timed(fwd_bwd(theirs), f.reps)
        torch.cuda.synchronize()
        with L.KernelTimer() as timer:
            fwd_bwd(ours)()
            torch.cuda.synchronize()
        kernels = [(name, round(ms * 1e3, 1)) for name, ms in timer.records]
        rec = dict(kind=kind, T=t, P=np_, N=nn, E=e, dimensions=k, fwd_us=t_f, fwd_bwd_us=t_fb,
                   bwd_us=t_fb - t_f, svdvals_fwd_us=t_fr, svdvals_fwd_bwd_us=t_fbr,
                   launches=len(kernels), kernels_us=kernels, loss=float(ours()), svdvals_loss=float(theirs()))
        out.append(rec)
        print('%-8s forward %8.1f us  forward+backward %8.1f us | svdvals autograd (float32) forward %9.1f us  '
              'forward+backward %9.1f us' % (kind, t_f, t_fb, t_fr, t_fbr))
        print('         %d launches: %s' % (len(kernels), ', '.join('%s %.1f' % kv for kv in kernels)))
    if f.json:
        for rec in out:
            print(json.dumps(rec))


if __name__ == '__main__':
    main()

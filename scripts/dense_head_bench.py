"""Times the dense reduction-head kernels (csrc/dense.hip) on the MI355X.

For every (M, K, N) of the grid: forward, backward-data and weight-gradient in microseconds (median
of --reps launches, HIP events around each), the fraction of 8 TB/s that streaming the bytes of W
(forward, backward-data) or of dW (weight gradient) once in that time would take, and torch.addmm
in float32 on the same operands next to it.  Then the whole 3fc train step of the head (forward,
backward, TFAdam) at the training batch.  One JSON line per row with --json.

    python scripts/dense_head_bench.py [--rows 4,25,50,192] [--reps 20] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd.model import reduction as R  # noqa: E402
from soft_contrastive_learning_amd.train.optim import make_optimizer  # noqa: E402

SHAPES = [(32768, 4096), (84480, 4096), (4096, 4096), (4096, 512), (32768, 512)]
PEAK = 8.0e12


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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--rows', default='4,25,50,192')
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--json', action='store_true')
    a = p.parse_args(argv)
    dev = torch.device('cuda:0')
    rows = [int(v) for v in a.rows.split(',')]
    out = []
    hdr = '%5s %6s %5s | %9s %5s %9s | %9s %5s %9s | %9s %5s %9s' % (
        'M', 'K', 'N', 'fwd us', 'of8T', 'addmm', 'bwd_d us', 'of8T', 'mm', 'wgrad us', 'of8T', 'mm')
    print(hdr)
    for K, N in SHAPES:
        w = torch.randn(K, N, device=dev)
        b = torch.randn(N, device=dev)
        gw = torch.empty_like(w)
        gb = torch.empty_like(b)
        wbytes = 4.0 * K * N
        for M in rows:
            x = torch.randn(M, K, device=dev)
            gy = torch.randn(M, N, device=dev)
            y = R.dense_fwd(x, w, b, True)
            t_f = timed(lambda: R.dense_fwd(x, w, b, True), a.reps)
            t_fr = timed(lambda: torch.addmm(b, x, w), a.reps)
            t_d = timed(lambda: R.dense_bwd_data(gy, y, w), a.reps)
            t_dr = timed(lambda: torch.mm(gy, w.t()), a.reps)
            t_w = timed(lambda: R.dense_wgrad(x, gy, y, gw, gb), a.reps)
            t_wr = timed(lambda: torch.mm(x.t(), gy, out=gw), a.reps)
            rec = dict(M=M, K=K, N=N, fwd_us=t_f, fwd_addmm_us=t_fr, bwd_data_us=t_d, bwd_data_mm_us=t_dr,
                       wgrad_us=t_w, wgrad_mm_us=t_wr, fwd_frac=wbytes / (t_f * 1e-6) / PEAK,
                       bwd_data_frac=wbytes / (t_d * 1e-6) / PEAK, wgrad_frac=wbytes / (t_w * 1e-6) / PEAK)
            out.append(rec)
            print('%5d %6d %5d | %9.1f %5.2f %9.1f | %9.1f %5.2f %9.1f | %9.1f %5.2f %9.1f' % (
                M, K, N, t_f, rec['fwd_frac'], t_fr, t_d, rec['bwd_data_frac'], t_dr, t_w, rec['wgrad_frac'],
                t_wr))
            del x, gy, y
        del w, b, gw, gb
        torch.cuda.empty_cache()
    # the whole 3fc head train step at the training batch (25 rows), both input widths
    for K in (32768, 84480):
        head = R.DenseHead('3fc', K, 512).to(dev)
        opt = make_optimizer('adam', list(head.parameters()), 5e-6)
        x = torch.randn(25, K, device=dev, requires_grad=True)
        coef = torch.randn(25, 512, device=dev)

        def fwd_bwd():
            for q in head.parameters():
                q.grad = None
            (head(x) * coef).sum().backward()

        def step():
            fwd_bwd()
            opt.step()
        t_fb = timed(fwd_bwd, a.reps)
        t_all = timed(step, a.reps)
        rec = dict(step='3fc', M=25, K=K, out_dim=512, fwd_bwd_us=t_fb, adam_us=t_all - t_fb, step_us=t_all)
        out.append(rec)
        print('3fc train step M=25 K=%d: forward+backward %.1f us, TFAdam %.1f us, total %.1f us' % (
            K, t_fb, t_all - t_fb, t_all))
        del head, opt, x
        torch.cuda.empty_cache()
    if a.json:
        for rec in out:
            print(json.dumps(rec))


if __name__ == '__main__':
    main()

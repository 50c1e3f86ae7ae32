"""Times the side-sized spectral losses (eigen_solve_kernel of csrc/spectral_loss.hip) on the
MI355X: residual_det, residual_trace, swrd and ntuplet_evmm.

At the trainer's shape (T = 2, P = N = 12, E = 32768, dimensions 10 by default), like
scripts/spectral_loss_bench.py: forward and forward + backward in microseconds (median of --reps
calls, HIP events around each, allocations and the Python of the autograd Function included) and
the kernels of one forward + backward with their own durations (KernelTimer).  Next to them, in
the same run:

* residual_det and swrd through ``wrd_loss`` with indicator / zero-padded weights — the same loss
  on the (P + N)-sized matrix, the only route before these kernels existed;
* the same loss on ``torch.linalg.svdvals`` / ``eigvalsh`` and autograd in float32 on the device.

ntuplet_evmm runs with a margin of 20 (lambda_max <= N + 1 on unit rows), so that every tuple's
hinge is active and the backward has work.  One JSON line per loss with --json.

    python scripts/eigen_loss_bench.py [--tuples 2] [--positives 12] [--negatives 12]
                                       [--width 32768] [--dimensions 10] [--reps 20] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.model import losses as M  # noqa: E402
from spectral_loss_bench import timed  # noqa: E402
from tests import spectral_data as D  # noqa: E402

KINDS = ('residual_det', 'residual_trace', 'swrd', 'ntuplet_evmm')
EVMM_MARGIN = 20.0


def torch_loss(kind, a, pos, neg, pw, nw, margin, k):
    """model/losses.py:317-327, 345-370, 613-624 on torch ops."""
    if kind == 'ntuplet_evmm':
        fp, fn = torch.cat([a, pos], 1), torch.cat([a, neg], 1)
        lp = torch.linalg.eigvalsh(fp @ fp.transpose(1, 2))[:, 0]
        ln = torch.linalg.eigvalsh(fn @ fn.transpose(1, 2))[:, -1]
        return torch.clamp(margin + lp - ln, min=0.0).mean(0)
    yp, yn = pos - a, neg - a
    if kind == 'swrd':
        yp, yn = yp * pw, yn * nw
    sp, sn = torch.linalg.svdvals(yp)[:, :k], torch.linalg.svdvals(yn)[:, :k]
    if kind == 'residual_trace':
        return (sp.sum(1) - sn.sum(1) + margin).mean(0)
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
    pwt = torch.tensor(pw[:, :np_], device=dev)[:, :, None].contiguous()
    nwt = torch.tensor(nw[:, np_:], device=dev)[:, :, None].contiguous()
    zero_p, zero_n = torch.zeros_like(pwt), torch.zeros_like(nwt)
    print('T=%d P=%d N=%d E=%d dimensions=%d: input %.1f MB' % (t, np_, nn, e, k, zt.numel() * 4 / 1e6))
    out = []
    for kind in KINDS:
        margin = EVMM_MARGIN if kind == 'ntuplet_evmm' else 0.1
        # the (P + N)-row weights under which wrd_loss computes the same loss
        wp, wn = (pwt, nwt) if kind == 'swrd' else (torch.ones_like(pwt), torch.ones_like(nwt))
        pad_p, pad_n = torch.cat([wp, zero_n], 1), torch.cat([zero_p, wn], 1)

        def ours():
            if kind == 'swrd':
                return M.swrd_loss(a, pos, neg, pwt, nwt, margin, dimensions=k)
            if kind == 'ntuplet_evmm':
                return M.ntuplet_evmm_loss(a, pos, neg, margin)
            return getattr(M, kind + '_loss')(a, pos, neg, margin, dimensions=k)

        def padded():
            return M.wrd_loss(a, pos, neg, pad_p, pad_n, margin, dimensions=k)

        def theirs():
            return torch_loss(kind, a, pos, neg, pwt, nwt, margin, k)

        def fwd_bwd(make):
            def go():
                for x in (a, pos, neg):
                    x.grad = None
                make().backward()
            return go

        routes = [('own', ours), ('torch', theirs)]
        if kind in ('residual_det', 'swrd'):
            routes.insert(1, ('wrd_padded', padded))
        rec = dict(kind=kind, T=t, P=np_, N=nn, E=e, dimensions=k, margin=margin)
        for name, fn in routes:
            with torch.no_grad():
                rec[name + '_fwd_us'] = timed(fn, f.reps)
            rec[name + '_fwd_bwd_us'] = timed(fwd_bwd(fn), f.reps)
            rec[name + '_loss'] = float(fn())
            torch.cuda.synchronize()
            if name != 'torch':
                with L.KernelTimer() as timer:
                    fwd_bwd(fn)()
                    torch.cuda.synchronize()
                rec[name + '_kernels_us'] = [(n, round(ms * 1e3, 1)) for n, ms in timer.records]
        out.append(rec)
        print('%-14s %s' % (kind, ' | '.join('%s forward %8.1f us forward+backward %8.1f us'
                                             % (n, rec[n + '_fwd_us'], rec[n + '_fwd_bwd_us']) for n, _ in routes)))
        for name in ('own', 'wrd_padded'):
            if name + '_kernels_us' in rec:
                ks = rec[name + '_kernels_us']
                print('    %-10s %d launches: %s' % (name, len(ks), ', '.join('%s %.1f' % kv for kv in ks)))
    if f.json:
        for rec in out:
            print(json.dumps(rec))


if __name__ == '__main__':
    main()

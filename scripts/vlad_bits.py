#!/usr/bin/env python
"""The bits of the NetVLAD head, for comparing two builds on one machine type: one line per case with
the SHA-256 of out, grad_x, grad_w, grad_c (ONE digest over the four tensors' bytes in that order;
inference: out alone) and the two *_workspace_bytes values.  The C-ABI is called
directly (as scripts/netvlad_wall.py does), inputs from tests/util_data.py.  Run it once from each
tree, each in a fresh process, and compare the outputs byte by byte; the slice count depends on the
CU count, so the hashes hold per machine type.

    python scripts/vlad_bits.py                 # the product library
    python scripts/vlad_bits.py --variant 922   # the diagnostic build under scl_debug_set_variant(922)

Cases: bf16 maps (1,1), (3,33), (2,165), (40,70), (5,1200), (2,2100), training (with the call's own
plane images and with planes handed in) and inference; (200,165) inference (the one-workgroup-per-
image form, B >= 144); float32 maps (1,1), (3,33), (2,64), (4,196), training and inference.  pre_l2
is on except at (2,165) and (2,64).
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_CASES = [(1, 1), (3, 33), (2, 165), (40, 70), (5, 1200), (2, 2100)]
F32_CASES = [(1, 1), (3, 33), (2, 64), (4, 196)]
NO_PRE_L2 = {(2, 165), (2, 64)}


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', type=int, default=0)
    args = ap.parse_args()
    if args.variant:
        os.environ['SCL_DIAG'] = '1'
    from soft_contrastive_learning_amd import _lib as L
    from tests import util_data as U

    dev = torch.device('cuda:0')
    lib = L.load()
    if args.variant:
        lib.scl_debug_set_variant(args.variant)

    def case(b, n, bf16, train, planes_in):
        pre_l2 = 0 if (b, n) in NO_PRE_L2 else 1
        x = U.feature_map(b, n, seed=7 * b + n)
        if not pre_l2:
            x = x * 0.1
        w, c = U.vlad_params(seed=8, logit_scale=3.0 if pre_l2 else 1.0)
        g = np.random.default_rng(2).standard_normal((b, 32768)).astype(np.float32)
        xt = torch.tensor(x, device=dev)
        if bf16:
            xt = xt.bfloat16()
        dt = L.DT_BF16 if bf16 else L.DT_F32
        wt, ct, go = torch.tensor(w, device=dev), torch.tensor(c, device=dev), torch.tensor(g, device=dev)
        out = torch.empty(b, 32768, device=dev)
        sa = sl = sr = sv = None
        if train:
            sa, sl = torch.empty(b, n, 64, device=dev), torch.empty(b, n, 64, device=dev)
            sr, sv = torch.empty(b, n, device=dev), torch.empty(b, L.VLAD_SAVE_ROWS, 64, device=dev)
        nf, nb = lib.scl_netvlad_fwd_workspace_bytes(b, n), lib.scl_netvlad_bwd_workspace_bytes(b, n)
        wsf, wsb = L.workspace(nf, dev), L.workspace(nb, dev)
        st = L.stream_of(xt)
        planes = None
        if planes_in:
            planes = torch.empty(lib.scl_netvlad_planes_bytes(), dtype=torch.uint8, device=dev)
            L.check(lib.scl_netvlad_planes(L.ptr(wt), L.ptr(planes), st))
        L.check(lib.scl_netvlad_fwd_p(L.ptr(xt), dt, L.ptr(wt), L.ptr(ct), L.ptr(planes), b, n, pre_l2, L.ptr(out),
                                      L.ptr(sa), L.ptr(sl), L.ptr(sr), L.ptr(sv), L.ptr(wsf), wsf.numel(), st))
        outs = [out]
        if train:
            gx, gw, gc = torch.empty_like(xt), torch.empty_like(wt), torch.empty_like(ct)
            L.check(lib.scl_netvlad_bwd_p(L.ptr(xt), dt, L.ptr(wt), L.ptr(ct), L.ptr(planes), L.ptr(go), L.ptr(sa),
                                          L.ptr(sl), L.ptr(sr), L.ptr(sv), b, n, pre_l2, L.ptr(gx), L.ptr(gw),
                                          L.ptr(gc), L.ptr(wsb), wsb.numel(), st))
            outs += [gx, gw, gc]
        torch.cuda.synchronize()
        print('variant %d  %-7s (%3d,%4d) %-9s pre_l2 %d  planes %-6s  sha256 %s  '
              'ws %d %d' % (args.variant, 'bf16' if bf16 else 'float32', b, n, 'training' if train else 'inference',
                            pre_l2, 'given' if planes_in else 'own', sha(outs), nf, nb), flush=True)

    try:
        for train in (True, False):
            for b, n in BF16_CASES:
                for planes_in in ((False, True) if train else (False,)):
                    case(b, n, True, train, planes_in)
        case(200, 165, True, False, False)
        for train in (True, False):
            for b, n in F32_CASES:
                case(b, n, False, train, False)
    finally:
        if args.variant:
            lib.scl_debug_set_variant(0)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Which kernel serves which convolution pass of the backbone, and what it computes.

For each case of ``case_list()`` one ``model.features`` forward (and backward) is run on seeded inputs and
recorded: the ordered kernel names of the project's own launches (``_lib.KernelTimer``: its sink is
process-wide, so the autograd thread's and the side stream's launches are in it), the ``WORK_LOG``
dictionary, the feature map and every parameter gradient.

  backbone_route_trace.py --out trace.json                 record the tree's nets.py (digests of the tensors)
  backbone_route_trace.py --nets OTHER.py --golden F.json  record another nets.py (loaded under a second module
                                                           name in the same package) and write the fixture of
                                                           tests/test_gpu_backbone_routes.py from it
  backbone_route_trace.py --against OTHER.py --out r.json  run every case on both and compare: launch lists and
                                                           WORK_LOG identical; tensors torch.equal, or — where a
                                                           library convolution takes part, whose kernels are not
                                                           promised bit-reproducible — within the case's row in
                                                           tests/test_gpu_switches.py.  Exit status 1 on a difference.

Reads nothing outside the tree."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from soft_contrastive_learning_amd import _lib as L, parallel          # noqa: E402
from soft_contrastive_learning_amd.model import nets as tree_nets      # noqa: E402
from tests import util_data                                            # noqa: E402
from tests.test_gpu_switches import ALL, CASES as SWITCH_CASES        # noqa: E402

SHAPES = [(2, 480, 640), (2, 180, 240), (3, 135, 241), (1, 16, 16)]
# the cases of the permanent test (tests/golden/backbone_routes_v1.json)
GOLDEN_SHAPES = SHAPES[:3]
# a library convolution in a case without a row of its own: the row of the deep layers through the library
LIBRARY_ROW = (3e-2, 0.4, ALL)


def case_name(shape, sink, extra=''):
    return '%dx%dx%d%s%s' % (shape + ('+sink' if sink else '', extra))


def case_list():
    """[(name, dict)]: shape, sink, flags, dtype, mode ('train' | 'no_grad' | 'first_layer'), and the
    tolerance row that holds where a library convolution takes part (None: none does — bit-identical)."""
    out = []
    for shape in SHAPES:
        for sink in (True, False):
            out.append((case_name(shape, sink),
                        dict(shape=shape, sink=sink, row=None if shape == SHAPES[0] else LIBRARY_ROW)))
    library = ('USE_WRW', 'USE_FIRST', 'USE_CONVG', 'USE_CONV64', 'USE_F32_WEIGHTS')
    for flags, row in SWITCH_CASES:
        name = case_name(SHAPES[0], True, ',' + '+'.join('%s=0' % k[4:] for k in flags))
        out.append((name, dict(shape=SHAPES[0], sink=True, flags=dict(flags),
                               row=row if any(k in library for k in flags) else None)))
    out.append((case_name(SHAPES[0], True, ',SPLIT_FWD=1'),
                dict(shape=SHAPES[0], sink=True, flags={'USE_SPLIT_FWD': True}, row=None)))
    out.append((case_name(SHAPES[0], False, ',no_grad'), dict(shape=SHAPES[0], sink=False, mode='no_grad', row=None)))
    out.append((case_name(SHAPES[1], True, ',float32'),
                dict(shape=SHAPES[1], sink=True, dtype=torch.float32, row=LIBRARY_ROW)))
    out.append((case_name(SHAPES[0], False, ',first_layer'),
                dict(shape=SHAPES[0], sink=False, mode='first_layer', row=None)))
    # ... and with its weight gradient from the library (the executor with need_x false)
    out.append((case_name(SHAPES[0], False, ',first_layer,FIRST=0'),
                dict(shape=SHAPES[0], sink=False, mode='first_layer', flags={'USE_FIRST': False}, row=LIBRARY_ROW)))
    return out


def load_nets(path):
    """Another nets.py under a second module name in the same package (its relative imports resolve)."""
    name = 'soft_contrastive_learning_amd.model._nets_other'
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def run_case(nets, dev, shape, sink=False, flags=None, dtype=torch.bfloat16, mode='train', row=None):
    """(ordered kernel names, WORK_LOG, {name: tensor}) of one pass."""
    b, h, w = shape
    flags = flags or {}
    img = torch.tensor(util_data.pose_images(b, h, w, seed=3), device=dev)
    old = {k: getattr(nets, k) for k in flags}
    buckets = None
    try:
        for k, v in flags.items():
            setattr(nets, k, v)
        model = nets.VGG16NetVLAD(compute_dtype=dtype, seed=9, fused_relu=True).to(dev)
        tensors = {}
        nets.WORK_LOG = {}
        if mode == 'no_grad':
            with L.KernelTimer() as kt, torch.no_grad():
                f = model.features(img)
                torch.cuda.synchronize()
        elif mode == 'first_layer':
            # conv1_1 alone, only its parameters want a gradient (need_x is false)
            wt, bias = model.conv1_1_kernel, model.conv1_1_bias
            with L.KernelTimer() as kt:
                f = nets._FirstConv.apply(img, model.average_rgb.detach(), wt, bias, dtype, None)
                g = torch.randn(f.shape, generator=torch.Generator().manual_seed(72)).to(dev).to(f.dtype)
                f.backward(g.contiguous(memory_format=torch.channels_last))
                torch.cuda.synchronize()
        else:
            params = [p for n, p in model.named_parameters() if not n.startswith(('assignment', 'cluster'))]
            if sink:
                buckets = parallel.GradBuckets(params)
                nets.GRAD_SINK = buckets
                buckets.zero()
            with L.KernelTimer() as kt:
                f = model.features(img)
                g = torch.randn(f.shape, generator=torch.Generator().manual_seed(72)).to(dev).to(f.dtype)
                f.backward(g)
                if sink:
                    buckets.finish()
                torch.cuda.synchronize()
        tensors['features'] = f.detach().float().clone()
        for n, p in model.named_parameters():
            if p.grad is not None:
                tensors['grad:' + n] = p.grad.detach().float().clone()
        return [name for name, _ in kt.records], nets.WORK_LOG, tensors
    finally:
        nets.GRAD_SINK = None
        nets.WORK_LOG = None
        if buckets is not None:
            buckets.close()
        for k, v in old.items():
            setattr(nets, k, v)


def digest(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def compare(mine, theirs, row):
    """(differences between two run_case results: [] = equal as required, largest norm-relative
    deviation of a tensor: 0.0 = all bit-identical)."""
    bad = []
    if mine[0] != theirs[0]:
        bad.append('launch lists differ: %s | %s' % (mine[0], theirs[0]))
    if mine[1] != theirs[1]:
        bad.append('WORK_LOG differs')
    if set(mine[2]) != set(theirs[2]):
        bad.append('tensor sets differ')
        return bad, float('nan')
    worst = 0.0
    for n, a in mine[2].items():
        b = theirs[2][n]
        if torch.equal(a, b):
            continue
        v = float((a - b).norm() / a.norm().clamp_min(1e-30))
        worst = max(worst, v)
        if row is None:
            bad.append('%s not bit-identical (%.3g)' % (n, v))
            continue
        ftol, gtol, loose = row
        tol = ftol if n == 'features' else (gtol if loose is None or n[len('grad:'):] in loose else 0.0)
        if not v <= tol:
            bad.append('%s differs by %.3g > %.3g' % (n, v, tol))
    return bad, worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--nets', help='record this nets.py instead of the tree\'s')
    ap.add_argument('--against', help='compare the tree\'s nets.py with this one, case by case')
    ap.add_argument('--golden', help='write the kernel-name lists of the default-switch cases here')
    ap.add_argument('--out', help='write the whole record (JSON) here')
    ap.add_argument('--only', help='run the cases whose name contains this')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda:0')
    nets = load_nets(args.nets) if args.nets else tree_nets
    other = load_nets(args.against) if args.against else None
    record, golden, failed = {}, {}, 0
    for name, case in case_list():
        if args.only and args.only not in name:
            continue
        got = run_case(nets, dev, **case)
        entry = {'launches': got[0], 'work_log': got[1], 'digests': {n: digest(t) for n, t in got[2].items()}}
        if other is not None:
            bad, worst = compare(got, run_case(other, dev, **case), case['row'])
            entry['against'] = {'differences': bad, 'largest_relative_deviation': worst}
            failed += bool(bad)
            print('%-60s %3d launches  %s' % (name, len(got[0]), 'DIFFERS: %s' % bad if bad else (
                'bit-identical' if worst == 0.0 else 'within the row (largest deviation %.3g)' % worst)), flush=True)
        else:
            print('%-60s %3d launches' % (name, len(got[0])), flush=True)
        record[name] = entry
        if case['shape'] in GOLDEN_SHAPES and not case.get('flags') and 'mode' not in case and 'dtype' not in case:
            golden[name] = got[0]
        del got
        torch.cuda.empty_cache()
    for path, what in ((args.out, record), (args.golden, golden)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                json.dump(what, f, indent=1, sort_keys=True)
                f.write('\n')
    if other is not None:
        print('%d of %d cases differ' % (failed, len(record)))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())

"""Measures queries with a position prior (evaluation/retrieval.RetrievalIndex.query(near=, radius=),
csrc/topn.hip scl_topn_index_query_window) on the MI355X against the un-windowed stream route of the
same index, in one process on one box.

R = 100 000 references, d = 256, n = 25, certified, Q in {1, 32} random queries.  The positions
are a traverse (1 m between consecutive rows), and the same rows with the positions permuted against
them, where no tile can be skipped.  Windows of about 1 %, 10 % and 100 % of the rows are centred
on consecutive frames of a drive past the middle of the list (4 m apart: the windows of one call
overlap, as a tracker's do).  Two passes, every case in turn in each:

* the C call alone, --reps calls of every case taken in turn with HIP events around each call and
  no read-back in between: medians, and the difference to the un-windowed call of the same Q;
* device time per kernel (``_lib.KernelTimer``: events around every launch), means of --reps calls.

The answers of every windowed case are compared with ``topn_l2`` on each query's gathered subset
before anything is timed (exit status 1 on a difference).  Nothing else is gated: the table is the
record that DESIGN.md quotes.

    python scripts/retrieval_window_bench.py [--reps 50] [--out profiles/retrieval_window/retrieval_window_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.evaluation import retrieval  # noqa: E402

R, D, N = 100000, 256, 25
QS = (1, 32)
SHARES = (0.01, 0.1, 1.0)
KERNELS = ('score', 'select', 'rerank')


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def events(reps):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]


def alternate_us(fns, reps, warmup=5):
    """Medians (us) of the calls of every function, taken in turn: f0, f1, f0, f1, .."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [events(reps) for _ in fns]
    for k in range(reps):
        for e, fn in zip(ev, fns):
            e[k][0].record()
            fn()
            e[k][1].record()
    torch.cuda.synchronize()
    return [median(a.elapsed_time(b) * 1e3 for a, b in e) for e in ev]


def raw_call(index, qt, n, near=None, radius=None):
    """The C call alone on buffers of its own: scl_topn_index_query, or _query_window with a window."""
    lib = L.load()
    ref = index.ref
    r, d = ref.shape
    q, dev = qt.shape[0], ref.device
    ws = L.workspace(lib.scl_topn_index_query_workspace_bytes(r, q, d, n, index._flags), dev)
    idx = torch.empty((q, n), dtype=torch.int64, device=dev)
    dist = torch.empty((q, n), dtype=torch.float64, device=dev)
    count = torch.empty(q, dtype=torch.int32, device=dev)
    flag = torch.empty(q, dtype=torch.uint8, device=dev)
    bound = torch.empty(q, dtype=torch.float64, device=dev)

    def plain():
        L.check(lib.scl_topn_index_query(L.ptr(ref), r, d, L.ptr(index._index), index._index.numel(),
                                         L.ptr(qt), q, n, 0, L.ptr(idx), L.ptr(dist), L.ptr(flag),
                                         L.ptr(bound), L.ptr(ws), ws.numel(), index._flags, L.stream_of(ref)))

    def windowed():
        L.check(lib.scl_topn_index_query_window(
            L.ptr(ref), r, d, L.ptr(index._index), index._index.numel(), L.ptr(index._geo), index._geo.numel(),
            L.ptr(qt), q, L.ptr(near), L.ptr(radius), n, 0, L.ptr(idx), L.ptr(dist), L.ptr(count), L.ptr(flag),
            L.ptr(bound), L.ptr(ws), ws.numel(), index._flags, L.stream_of(ref)))
    return plain if near is None else windowed


def kernel_us(fn, reps):
    """Mean device time (us) per launch of the three kernels of one call, by the library's own events."""
    with L.KernelTimer(capacity=4 * reps + 16) as kt:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = dict.fromkeys(KERNELS, 0.0)
    for name, (_, ms) in kt.summary().items():
        for k in KERNELS:
            if k in name:
                out[k] += ms * 1e3
    return out


def subset_answers_differ(index, xy, qt, near, radius, got):
    """Does any row differ from topn_l2 on the gathered subset (the specification)?"""
    dist, idx = got
    for k in range(qt.shape[0]):
        dx, dy = xy[:, 0] - near[k, 0], xy[:, 1] - near[k, 1]
        w = torch.nonzero((radius[k] >= 0) & (dx * dx + dy * dy <= radius[k] * radius[k])).reshape(-1)
        m = min(N, w.numel())
        if m:
            dd, ii = retrieval.topn_l2(index.ref[w].contiguous(), qt[k:k + 1], m)
            if not (torch.equal(dist[k, :m], dd[0]) and torch.equal(idx[k, :m], w[ii[0]])):
                return True
        if not (bool((idx[k, m:] == -1).all()) and bool(torch.isinf(dist[k, m:]).all())):
            return True
    return False


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'retrieval_window_bench.py measures on a HIP device'
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs, %.0f GB; torch %s, HIP %s'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                prop.total_memory / 1e9, torch.__version__, torch.version.hip),
             'R = %d, d = %d, n = %d, certified, float32 scores; %d calls per case, the cases of one Q in turn'
             % (R, D, N, f.reps),
             'call: median us of the C call alone, HIP events around each call; score / select / rerank: mean '
             'device us per launch (events around every launch, a pass of its own)']
    gen = torch.Generator(device=dev).manual_seed(11)
    ref = torch.randn(R, D, generator=gen, device=dev)
    qry = torch.randn(max(QS), D, generator=gen, device=dev)
    j = torch.arange(R, dtype=torch.float64, device=dev)
    track = torch.stack([620000.25 + j, 5735000.5 + 0.5 * torch.sin(j / 50.0)], 1)
    layouts = (('traverse', track), ('permuted', track[torch.randperm(R, generator=gen, device=dev)]))
    ok = True
    for q in QS:
        qt = qry[:q].contiguous()
        cases = []                                       # (label, C call, [Q] window sizes or None)
        for name, xy in layouts:
            index = retrieval.RetrievalIndex(ref, 0, 'f32', positions=xy)
            if name == 'traverse':
                cases.append(('no window', raw_call(index, qt, N), None))
            for share in SHARES:
                rows = R // 2 + 4 * torch.arange(q, device=dev)                 # a drive: 4 m between frames
                near = track[rows].contiguous()
                radius = torch.full((q,), 1e9 if share == 1.0 else share * R / 2.0, dtype=torch.float64, device=dev)
                st = {}
                got = index.query(qt, N, stats=st, near=near, radius=radius)
                bad = subset_answers_differ(index, xy, qt, near, radius, got) or st['uncertified'] != 0
                ok = ok and not bad
                dx, dy = xy[:, None, 0] - near[None, :, 0], xy[:, None, 1] - near[None, :, 1]
                sizes = (dx * dx + dy * dy <= radius * radius).sum(0)
                cases.append(('%s %3.0f %%%s' % (name, 100 * share, '  RESULTS DIFFER' if bad else ''),
                              raw_call(index, qt, N, near, radius), sizes))
        calls = alternate_us([c[1] for c in cases], f.reps)
        base = calls[0]
        for (label, fn, sizes), us in zip(cases, calls):
            k = kernel_us(fn, f.reps)
            lines.append('Q = %2d  %-15s  rows per window %7s   call %7.1f us (%+7.1f)   score %7.1f   select %6.1f   '
                         'rerank %6.1f   largest: %s'
                         % (q, label, '-' if sizes is None else '%.0f' % float(sizes.double().mean()), us, us - base,
                            k['score'], k['select'], k['rerank'], max(KERNELS, key=k.get)))
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

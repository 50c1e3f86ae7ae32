"""Measures the resident index for descriptors wider than 256 columns
(evaluation/retrieval.RetrievalIndex(wide='resident'), csrc/topn.hip scl_topn_wide_query) on the
MI355X against the delegated route of the same rows (wide='delegate': ``topn_l2`` per call, what
every wide query took before), in one process on one box.

R = 100 000 references, d in {512, 1024, 4096}, n = 25, certified, Q in {1, 32} random queries, and
a window of 1 % of the rows on a traverse (1 m between consecutive rows, the frames of a call 4 m
apart).  Per (d, Q), every case in turn:

* ``query``: median host time of ``RetrievalIndex.query`` ending in a device synchronise — the
  delegated route synchronises inside, so only a host clock measures both alike;
* ``C call``: median of the resident C call alone, HIP events around each call;
* per kernel: mean device time per launch (``_lib.KernelTimer``: events around every launch of the
  library, a pass of its own).  The delegated route's torch launches are not the library's and are
  not in that column; its row gives the library launches per call and their summed time.

The score kernel's rate is R d 4 bytes over its time, beside the rate of the d <= 256 stream score
kernel on the first 256 columns of the same rows in the same run.  Before anything is timed the
resident answers are compared with the delegated ones (equal indices, nothing uncertified; exit
status 1 otherwise).  Nothing else is gated: the table is the record that DESIGN.md quotes.

    python scripts/retrieval_wide_bench.py [--reps 30] [--out profiles/retrieval_wide/retrieval_wide_bench.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.evaluation import retrieval  # noqa: E402

R, N = 100000, 25
DS = (512, 1024, 4096)
QS = (1, 32)
SHARE = 0.01
KERNELS = ('score', 'select', 'rerank')


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def host_us(fns, reps, warmup=3):
    """Medians (us) of host time around every function, each ending in a synchronise, taken in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for o, fn in zip(out, fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            o.append((time.perf_counter() - t0) * 1e6)
    return [median(o) for o in out]


def event_us(fns, reps, warmup=5):
    """Medians (us) of the calls of every function between HIP events, taken in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for _ in fns]
    for k in range(reps):
        for e, fn in zip(ev, fns):
            e[k][0].record()
            fn()
            e[k][1].record()
    torch.cuda.synchronize()
    return [median(a.elapsed_time(b) * 1e3 for a, b in e) for e in ev]


def raw_call(index, qt, n, near=None, radius=None):
    """The resident C call alone on buffers of its own: scl_topn_wide_query, with or without windows."""
    lib = L.load()
    ref = index.ref
    r, d = ref.shape
    q, dev = qt.shape[0], ref.device
    ws = L.workspace(lib.scl_topn_wide_query_workspace_bytes(r, q, d, n), dev)
    idx = torch.empty((q, n), dtype=torch.int64, device=dev)
    dist = torch.empty((q, n), dtype=torch.float64, device=dev)
    count = torch.empty(q, dtype=torch.int32, device=dev)
    flag = torch.empty(q, dtype=torch.uint8, device=dev)
    bound = torch.empty(q, dtype=torch.float64, device=dev)
    win = near is not None
    geo = (L.ptr(index._geo), index._geo.numel()) if win else (None, 0)

    def call():
        L.check(lib.scl_topn_wide_query(
            L.ptr(ref), r, d, L.ptr(index._index), index._index.numel(), *geo, L.ptr(qt), q,
            L.ptr(near) if win else None, L.ptr(radius) if win else None, n, 0, L.ptr(idx), L.ptr(dist),
            L.ptr(count) if win else None, L.ptr(flag), L.ptr(bound), L.ptr(ws), ws.numel(), L.stream_of(ref)))
    return call


def kernel_us(fn, reps):
    """(mean device us per call of each of the three stream kernels, library launches per call, their
    summed us per call), by the library's own events."""
    with L.KernelTimer(capacity=64 * reps + 64) as kt:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = dict.fromkeys(KERNELS, 0.0)
    launches, total = 0, 0.0
    for name, (count, ms) in kt.summary().items():
        launches += count
        total += count * ms * 1e3
        for k in KERNELS:
            if k in name:
                out[k] += count * ms * 1e3 / reps
    return out, launches / reps, total / reps


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=30)
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'retrieval_wide_bench.py measures on a HIP device'
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs, %.0f GB; torch %s, HIP %s'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                prop.total_memory / 1e9, torch.__version__, torch.version.hip),
             'R = %d, n = %d, certified, float32 scores; %d calls per case, the cases of one (d, Q) in turn' % (R, N, f.reps),
             'query: median host us of RetrievalIndex.query + synchronise; C call: median us between HIP events; '
             'score / select / rerank: mean device us per call (events around every library launch, a pass of its own)']
    gen = torch.Generator(device=dev).manual_seed(11)
    j = torch.arange(R, dtype=torch.float64, device=dev)
    track = torch.stack([620000.25 + j, 5735000.5 + 0.5 * torch.sin(j / 50.0)], 1)
    ok = True
    slower = []
    for d in DS:
        ref = torch.randn(R, d, generator=gen, device=dev)
        qry = torch.randn(max(QS), d, generator=gen, device=dev)
        resident = retrieval.RetrievalIndex(ref, 0, 'f32', positions=track, wide='resident')
        delegate = retrieval.RetrievalIndex(ref, 0, 'f32', positions=track)
        narrow = retrieval.RetrievalIndex(ref[:, :256].contiguous(), 0, 'f32')
        for q in QS:
            qt = qry[:q].contiguous()
            near = track[R // 2 + 4 * torch.arange(q, device=dev)].contiguous()       # a drive: 4 m between frames
            radius = torch.full((q,), SHARE * R / 2.0, dtype=torch.float64, device=dev)
            st = {}
            got = resident.query(qt, N, stats=st)
            want = delegate.query(qt, N)
            bad = not torch.equal(got[1], want[1]) or st['uncertified'] != 0 or st['route'] != 'wide'
            sw = {}
            resident.query(qt, N, stats=sw, near=near, radius=radius)
            bad = bad or sw['uncertified'] != 0 or sw['route'] != 'window'
            ok = ok and not bad
            t_del, t_res, t_win = host_us([lambda: delegate.query(qt, N), lambda: resident.query(qt, N),
                                           lambda: resident.query(qt, N, near=near, radius=radius)], f.reps)
            plain, windowed = raw_call(resident, qt, N), raw_call(resident, qt, N, near, radius)
            qn = qt[:, :256].contiguous()
            c_res, c_win = event_us([plain, windowed], f.reps)
            k_res, l_res, _ = kernel_us(plain, f.reps)
            k_win, l_win, _ = kernel_us(windowed, f.reps)
            k_del, l_del, s_del = kernel_us(lambda: delegate.query(qt, N), max(f.reps // 3, 3))
            k_nar, _, _ = kernel_us(lambda: narrow.query(qn, N), f.reps)
            if not t_res < t_del:
                slower.append((d, q))
            head = 'd = %4d  Q = %2d  ' % (d, q)
            lines.append(head + 'delegated         query %9.1f us                      library launches per call %5.1f, '
                         '%9.1f us of device time (torch launches not counted)%s'
                         % (t_del, l_del, s_del, '  RESULTS DIFFER' if bad else ''))
            for label, t, c, k, n_l in (('resident', t_res, c_res, k_res, l_res),
                                        ('resident, 1 % window', t_win, c_win, k_win, l_win)):
                lines.append(head + '%-17s query %9.1f us (%5.1f x)   C call %8.1f us   score %8.1f   select %6.1f   '
                             'rerank %7.1f   launches %.0f   largest: %s'
                             % (label, t, t_del / t, c, k['score'], k['select'], k['rerank'], n_l,
                                max(KERNELS, key=k.get)))
            lines.append(head + 'score kernel: %.2f TB/s over the %d-column rows; the d <= 256 stream score kernel on their '
                         'first 256 columns: %.1f us, %.2f TB/s'
                         % (R * d * 4 / k_res['score'] / 1e6, d, k_nar['score'], R * 256 * 4 / k_nar['score'] / 1e6))
        del resident, delegate, narrow, ref
    lines.append('resident faster than delegated (RetrievalIndex.query, host time) at every measured (d, Q): %s'
                 % ('yes' if not slower else 'NO, slower at %s' % slower))
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

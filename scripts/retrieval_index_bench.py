"""Measures queries against a prepared retrieval index (evaluation/retrieval.RetrievalIndex,
csrc/topn.hip scl_topn_index_query) on the MI355X against the one-shot call it replaces for a
resident reference set, in one process on one box.

R = 100 000 references, d = 256, n = 25, certified, Q in {1, 8, 32, 33, 128} random queries.  Per Q,
alternating, with HIP events around each call, medians of --reps calls after a warm-up:

* ``RetrievalIndex.query`` — Q <= 32: the stream route (score, select, re-rank); more: the scan fed
  from the index;
* ``retrieval.topn_l2`` — the yardstick of THIS run (norms, and planes with --score bf16x3, per call).

Both calls end with the read-back of the certificate flags, so both figures include one host
round trip.  A third figure leaves it out for the index: ``scl_topn_index_query`` alone, --reps
calls queued without a wait in between.  The stream route must move R d 4 bytes of reference rows
once and write and read the [Q][R] float32 score matrix; the achieved rate of that over the queued
time is printed with its share of 6.3 TB/s (one pass over 102 MB that is queried again and again
sits in the 256 MiB Infinity Cache: the rate is not an HBM rate).  The index build is timed once.

Expectations stated and checked (exit status 1 when missed): at every Q the index query takes no
longer than 1.05 x topn_l2 of the same run.

    python scripts/retrieval_index_bench.py [--reps 50] [--score f32] [--out profiles/retrieval_index/retrieval_index_bench.txt]
    python scripts/retrieval_index_bench.py --only-topn-l2      # the yardstick alone (A/B of two library builds)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.evaluation import retrieval  # noqa: E402

MARGIN = 1.05      # the run-to-run and box-to-box spread this project reports is +- 4 %
R, D, N = 100000, 256, 25
QS = (1, 8, 32, 33, 128)
PEAK_TBS = 6.3


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


def raw_query(index, qt, n):
    """scl_topn_index_query alone on the index's own buffers: no read-back between calls."""
    lib = L.load()
    ref = index.ref
    r, d = ref.shape
    q = qt.shape[0]
    ws = L.workspace(lib.scl_topn_index_query_workspace_bytes(r, q, d, n, index._flags), ref.device)
    idx = torch.empty((q, n), dtype=torch.int64, device=ref.device)
    dist = torch.empty((q, n), dtype=torch.float64, device=ref.device)
    flag = torch.empty(q, dtype=torch.uint8, device=ref.device)
    bound = torch.empty(q, dtype=torch.float64, device=ref.device)

    def call():
        L.check(lib.scl_topn_index_query(L.ptr(ref), r, d, L.ptr(index._index), index._index.numel(),
                                         L.ptr(qt), q, n, 0, L.ptr(idx), L.ptr(dist), L.ptr(flag),
                                         L.ptr(bound), L.ptr(ws), ws.numel(), index._flags,
                                         L.stream_of(ref)))
    return call


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--score', default='f32', choices=sorted(retrieval.SCORE_MODES))
    p.add_argument('--only-topn-l2', action='store_true', help='time the one-shot call alone')
    p.add_argument('--out', default='', help='also write the table to this file')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'retrieval_index_bench.py measures on a HIP device'
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    lines = ['box: %s (%s), %d CUs, %.0f GB; torch %s, HIP %s'
             % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
                prop.total_memory / 1e9, torch.__version__, torch.version.hip)]
    gen = torch.Generator(device=dev).manual_seed(11)
    ref = torch.randn(R, D, generator=gen, device=dev)
    qry = torch.randn(max(QS), D, generator=gen, device=dev)
    lines.append('R = %d, d = %d, n = %d, certified, score=%s; medians of %d calls, HIP events around each '
                 'call, the two calls in turn' % (R, D, N, f.score, f.reps))
    ok = True
    if f.only_topn_l2:
        for q in QS:
            qt = qry[:q].contiguous()
            us, = alternate_us([lambda: retrieval.topn_l2(ref, qt, N, 0, f.score)], f.reps)
            lines.append('Q = %3d   topn_l2 %9.1f us' % (q, us))
    else:
        torch.cuda.synchronize()
        a, b = events(1)[0]
        a.record()
        index = retrieval.RetrievalIndex(ref, 0, f.score)
        b.record()
        torch.cuda.synchronize()
        lines.append('index build (first call, includes its allocation): %.1f us, %d bytes'
                     % (a.elapsed_time(b) * 1e3, index._index.numel()))
        for q in QS:
            qt = qry[:q].contiguous()
            st = {}
            got = index.query(qt, N, stats=st)
            want = retrieval.topn_l2(ref, qt, N, 0, f.score)
            same = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            t_idx, t_l2 = alternate_us([lambda: index.query(qt, N),
                                        lambda: retrieval.topn_l2(ref, qt, N, 0, f.score)], f.reps)
            t_raw, = alternate_us([raw_query(index, qt, N)], f.reps)
            ratio = t_idx / t_l2
            met = ratio <= MARGIN and same and st['uncertified'] == 0
            ok = ok and met
            line = ('Q = %3d  %-6s  index.query %8.1f us   topn_l2 %8.1f us   ratio %.3f (expected <= %.2f): %s'
                    '   C call queued %8.1f us' % (q, st['route'], t_idx, t_l2, ratio, MARGIN,
                                                   'met' if met else 'MISSED', t_raw))
            if st['route'] == 'stream':
                nbytes = R * D * 4 + 2 * q * R * 4
                tbs = nbytes / t_raw / 1e6
                line += '   %5.1f MB -> %.2f TB/s, %.0f %% of %.1f' % (nbytes / 1e6, tbs, 100 * tbs / PEAK_TBS, PEAK_TBS)
            if not same:
                line += '   RESULTS DIFFER'
            lines.append(line)
    text = '\n'.join(lines)
    print(text)
    if f.out:
        os.makedirs(os.path.dirname(os.path.abspath(f.out)), exist_ok=True)
        with open(f.out, 'w') as fh:
            fh.write(text + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())

"""Geographic ground truth: the device route (evaluation/geo.py, csrc/geo_eval.hip) against the host
route it replaces, in one run.

    python scripts/geo_eval_bench.py --out profiles/geo_eval/geo_eval_bench.txt

100 000 references in traverse order at UTM magnitudes, Q = 1, 32, 1000 and 10 000 queries near
them, 25 hits per query.  Per Q, in this order (``ru_maxrss`` only ever grows, so everything on the
device route, at every Q, runs before the first host table exists):

  device  ``scl_geo_nearest`` and ``scl_geo_hit_dist`` on resident tensors, by device events (one pair
          per call, median and minimum over --reps calls after a warm-up), and
          ``top_n.device_ground_truth`` — query positions up, both calls, results down, the payload's
          lists built — by the host clock around a device synchronise;
  host    what evaluation/top-n.py:110-117 does and the parent did: ``pairwise_distances`` (the [Q, R]
          float64 table), the column gather ``[:, ref_idx]``, argmin / min, the Q x n lookup loop and
          the index translation, each by the host clock.  Skipped at a Q whose table and copy
          (16 Q R bytes) do not fit in three quarters of the available memory; the line says so.

Both routes' results are compared where both ran: the distances against the expanded form's error
bound, and the nearest rows — where the two routes name different ones,
the line gives the direct-form distance of the table's pick minus the device's (never negative: the
table's centimetres chose a reference that is farther away).  Peak resident memory of the process
after each section is ``ru_maxrss``.

Then ``top_n.main`` and ``localize.main`` end to end with ``--geo device`` and ``--geo table`` on one
synthetic set (--script_refs references, --script_queries queries), by the host clock.
"""
import argparse
import os
import resource
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.evaluation import geo, localize, top_n  # noqa: E402
from soft_contrastive_learning_amd.util import io as sio  # noqa: E402

N_HITS = 25


def traverse(n, seed):
    rng = np.random.default_rng(seed)
    head = np.cumsum(rng.normal(0.0, 0.02, n))
    step = rng.uniform(0.2, 3.0, n)
    return np.array([620000.0, 5700000.0]) + np.cumsum(np.stack([step * np.cos(head), step * np.sin(head)], 1), 0)


def rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def available_bytes():
    for line in open('/proc/meminfo'):
        if line.startswith('MemAvailable:'):
            return int(line.split()[1]) * 1024
    return 0


def event_times(fn, reps, warmup=5):
    """Milliseconds of ``reps`` calls of fn(), one event pair each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in pairs])


def device_section(emit, ref_dev, ref_idx, qxy, hits, reps):
    q = len(qxy)
    r = ref_dev.shape[0]
    lib = L.load()
    qt = torch.from_numpy(qxy).to(ref_dev.device)
    ht = torch.from_numpy(hits).to(ref_dev.device)
    idx = torch.empty(q, dtype=torch.int64, device=ref_dev.device)
    dist = torch.empty(q, dtype=torch.float64, device=ref_dev.device)
    out = torch.empty((q, N_HITS), dtype=torch.float64, device=ref_dev.device)
    nbytes = lib.scl_geo_nearest_workspace_bytes(r, q)
    ws = L.workspace(nbytes, ref_dev.device)
    st = L.stream_of(ref_dev)

    def nearest():
        L.check(lib.scl_geo_nearest(L.ptr(ref_dev), r, L.ptr(qt), q, L.ptr(idx), L.ptr(dist), L.ptr(ws),
                                    ws.numel(), st))

    def hit_dist():
        L.check(lib.scl_geo_hit_dist(L.ptr(ref_dev), r, L.ptr(qt), q, L.ptr(ht), N_HITS, L.ptr(out), st))

    tn, th = event_times(nearest, reps), event_times(hit_dist, reps)
    plan = geo.plan(r, q)
    emit('Q=%-6d device  scl_geo_nearest   median %9.1f us  min %9.1f us   (%s route, %d splits of %d rows, '
         'workspace %d bytes; %.2f G pairs/s at the median)'
         % (q, 1e3 * np.median(tn), 1e3 * tn.min(), plan['route'], plan['splits'], plan['split_rows'], nbytes,
            q * r / (1e6 * np.median(tn))))
    emit('Q=%-6d device  scl_geo_hit_dist  median %9.1f us  min %9.1f us   (n = %d)'
         % (q, 1e3 * np.median(th), 1e3 * th.min(), N_HITS))
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = top_n.device_ground_truth(ref_dev, qxy, ht, ref_idx)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    emit('Q=%-6d device  payload parts from host positions (upload, both calls, download, lists): median %9.3f ms'
         '   peak RSS %.0f MB' % (q, 1e3 * np.median(walls), rss_mb()))
    return parts, float(np.median(walls))


def host_section(emit, ref_xy, ref_idx, qxy, hits):
    from sklearn.metrics import pairwise_distances
    q = len(qxy)
    t = [time.perf_counter()]
    full = pairwise_distances(qxy, ref_xy, metric='euclidean')
    t.append(time.perf_counter())
    xy_dists = full[:, ref_idx]
    t.append(time.perf_counter())
    gt_i = np.argmin(xy_dists, axis=1)
    gt_g = np.min(xy_dists, axis=1)
    t.append(time.perf_counter())
    top_i = hits.astype(int)
    top_g = [[xy_dists[k, j] for j in top_i[k, :]] for k in range(q)]
    t.append(time.perf_counter())
    top_i = [[ref_idx[j] for j in top_i[k, :]] for k in range(q)]
    gt_i = [ref_idx[j] for j in gt_i]
    t.append(time.perf_counter())
    d = np.diff(t)
    emit('Q=%-6d host    table %9.3f ms  gather %9.3f ms  argmin/min %9.3f ms  lookup loop %9.3f ms  '
         'translate %9.3f ms  total %9.3f ms   peak RSS %.0f MB'
         % (q, 1e3 * d[0], 1e3 * d[1], 1e3 * d[2], 1e3 * d[3], 1e3 * d[4], 1e3 * d.sum(), rss_mb()))
    return (top_i, top_g, gt_i, gt_g), float(d.sum())


def compare(emit, q, dev_parts, host_parts, ref_xy, qxy):
    (d_top_i, d_top_g, d_gt_i, d_gt_g), (h_top_i, h_top_g, h_gt_i, h_gt_g) = dev_parts, host_parts
    u = 2.0 ** -53
    q2 = (qxy ** 2).sum(-1)
    # where the two routes name different nearest references, the table's centimetres decided: in the
    # direct form the table's pick must be no nearer than the device's
    d_gt, h_gt = np.asarray(d_gt_i), np.asarray(h_gt_i)
    differ = np.nonzero(d_gt != h_gt)[0]

    def direct(rows):
        dx, dy = ref_xy[rows, 0] - qxy[differ, 0], ref_xy[rows, 1] - qxy[differ, 1]
        return np.sqrt(dx * dx + dy * dy)
    same_gt = '%d of %d differ' % (len(differ), q) if len(differ) else 'all equal'
    if len(differ):
        gap = direct(h_gt[differ]) - direct(d_gt[differ])
        same_gt += ' (direct-form distance of the table\'s pick minus the device\'s: %.3g .. %.3g m)' % (gap.min(), gap.max())
    bound = 8 * u * (q2 + (ref_xy[np.asarray(d_gt_i)] ** 2).sum(-1)) + 8 * u * d_gt_g ** 2
    err = np.abs(d_gt_g ** 2 - h_gt_g ** 2)
    hb = 8 * u * (q2[:, None] + (ref_xy[np.asarray(d_top_i)] ** 2).sum(-1)) + 8 * u * np.asarray(d_top_g) ** 2
    herr = np.abs(np.asarray(d_top_g) ** 2 - np.asarray(h_top_g) ** 2)
    emit('Q=%-6d check   gt_i: %s   top_i equal: %s   max |table - direct| = %.4g m (gt), %.4g m (hits)   '
         'max |table^2 - direct^2| / bound = %.3f (gt), %.3f (hits)'
         % (q, same_gt, d_top_i == h_top_i, np.abs(d_gt_g - h_gt_g).max(),
            np.abs(np.asarray(d_top_g) - np.asarray(h_top_g)).max(), (err / bound).max(), (herr / hb).max()))


def script_section(emit, n_ref, n_query, workdir):
    """top_n.main and localize.main, files in -> pickle out, with both --geo values."""
    rng = np.random.default_rng(9)
    e, d = 64, 32
    ref_xy = traverse(n_ref, 5)
    pick = rng.integers(0, n_ref, n_query)
    qxy = ref_xy[pick] + rng.normal(0.0, 2.0, (n_query, 2))
    freq = rng.normal(0.0, 1.0 / 15.0, (2, 48))
    phase = rng.uniform(0.0, 2 * np.pi, 48)
    mix = rng.standard_normal((48, e))

    def feats(xy):
        f = np.cos((xy - ref_xy[0]) @ freq + phase) @ mix + 0.05 * rng.standard_normal((len(xy), e))
        return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)

    files = []
    for name, xy in (('ref', ref_xy), ('query', qxy)):
        path = os.path.join(workdir, 'set_%s.csv' % name)
        sio.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]], 'northing': [repr(float(v)) for v in xy[:, 1]]}, path)
        files += ['--%s_csv' % name, path]
    for name, f in (('pca', feats(ref_xy[::8])), ('ref', feats(ref_xy)), ('query', feats(qxy))):
        path = os.path.join(workdir, 'set_%s.v1.pickle' % name)
        sio.save_pickle([row for row in f], path)
        files += ['--%s_lv_pickle' % name, path]
    emit('scripts: %d references, %d queries, %d-wide descriptors whitened to %d, N = %d' % (n_ref, n_query, e, d, N_HITS))
    for name, main, extra in (('top_n.main', top_n.main, ['--D', str(d), '--L', '0.0']),
                              ('localize.main --batch 32', localize.main, ['--D', str(d), '--L', '0.0', '--batch', '32'])):
        payloads = {}
        for round_ in range(2):                        # the first round also pays every first launch
            for route in ('device', 'table'):
                out_root = os.path.join(workdir, '%s_%s_%d' % (name.split('.')[0], route, round_))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = main(files + ['--N', str(N_HITS), '--out_root', out_root, '--geo', route] + extra)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                path = written[0] if isinstance(written, list) else written
                payloads[route] = sio.load_pickle(path)
                if round_:
                    emit('%-26s --geo %-6s  %9.3f s   peak RSS %.0f MB' % (name, route, dt, rss_mb()))
        dv, tb = payloads['device'], payloads['table']
        emit('%-26s top_i equal: %s  top_f_dists equal: %s  gt_i: %d of %d differ  max |gt_g_dist table - device| = %.4g m'
             % (name, dv[0] == tb[0], bool(np.array_equal(dv[2], tb[2])), int((np.asarray(dv[3]) != np.asarray(tb[3])).sum()),
                len(dv[3]), np.abs(dv[4] - tb[4]).max()))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--refs', type=int, default=100000)
    p.add_argument('--queries', default='1,32,1000,10000')
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--script_refs', type=int, default=20000)
    p.add_argument('--script_queries', type=int, default=2000)
    p.add_argument('--out', default='', help='also write the table to this file')
    flags = p.parse_args(argv)
    assert torch.cuda.is_available(), 'this benchmark needs a HIP device'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device('cuda:0')
    props = torch.cuda.get_device_properties(dev)
    emit('%s, %d CUs; %d CPUs for this process; %.0f GB of host memory available'
         % (props.name, props.multi_processor_count, len(os.sched_getaffinity(0)), available_bytes() / 2 ** 30))
    emit('%d references in traverse order, %d hits per query; device times by events over %d calls'
         % (flags.refs, N_HITS, flags.reps))
    ref_xy = traverse(flags.refs, 1)
    ref_idx = [0] + list(range(flags.refs))              # l = 0: the loop's doubled row 0
    thinned = ref_xy[ref_idx]
    ref_dev = torch.from_numpy(thinned).to(dev)
    qs = [int(v) for v in flags.queries.split(',')]
    rng = np.random.default_rng(2)
    sets = {}
    for q in qs:
        at = rng.integers(0, flags.refs, q)
        qxy = ref_xy[at] + rng.normal(0.0, 2.0, (q, 2))
        hits = np.clip(at[:, None] + rng.integers(-40, 40, (q, N_HITS)), 0, flags.refs).astype(np.int64)
        sets[q] = (qxy, hits)
    emit('start: peak RSS %.0f MB' % rss_mb())
    results = {}
    for q in qs:
        results[q] = device_section(emit, ref_dev, ref_idx, sets[q][0], sets[q][1], flags.reps)
    for q in qs:
        need = 16 * q * len(ref_idx)
        if need > 0.75 * available_bytes():
            emit('Q=%-6d host    skipped: the table and its copy need %.1f GB, %.1f GB are available'
                 % (q, need / 2 ** 30, available_bytes() / 2 ** 30))
            continue
        host_parts, host_s = host_section(emit, ref_xy, ref_idx, sets[q][0], sets[q][1])
        compare(emit, q, results[q][0], host_parts, ref_xy, sets[q][0])
        emit('Q=%-6d host route / device route = %.0f x' % (q, host_s / results[q][1]))
        del host_parts
    with tempfile.TemporaryDirectory() as workdir:
        script_section(emit, flags.script_refs, flags.script_queries, workdir)
    if flags.out:
        os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
        with open(flags.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

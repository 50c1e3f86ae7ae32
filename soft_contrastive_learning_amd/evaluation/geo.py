"""Geographic ground truth and hit distances without the [Q, R] table.

The reference's ``evaluation/top-n.py`` builds ``pairwise_distances(query_xy, ref_xy)`` and reads
three things out of it (:110-113): the distance of every hit, the nearest reference of every
query and its distance.  This module computes those three from the positions themselves, on the
device that already holds the hit lists (csrc/geo_eval.hip).

**Definition** (``nearest_np`` / ``hit_distances_np`` are its executable statement; the kernels
give the same bits): ``d2(q, j) = dx*dx + dy*dy`` with ``dx = x_j - qx``, ``dy = y_j - qy`` in
float64, every operation rounded on its own (no fused multiply-add) — the direct form, not the
expansion ``|q|^2 + |r|^2 - 2 q.r`` scikit-learn's table uses, which loses centimetres to
cancellation at UTM magnitudes.

* ``nearest``: the lexicographically smallest ``(d2, j)``: a tie goes to the lower row
  (``np.argmin``'s choice) and the winner is decided on ``d2``, never on its root (distinct ``d2``
  often share one).  ``dist = sqrt(d2)``.  A NaN ``d2`` never wins, ``+inf`` can; where nothing
  wins (every ``d2`` is NaN) the row is ``-1`` and the distance ``+inf``.
* ``hit_distances``: ``sqrt(d2(q, idx[q, k]))`` for ``0 <= idx < R``, ``+inf`` for every other
  index (the ``-1`` a windowed query pads with, anything out of range).

``plan(R, Q)`` names the granules of ``scl_geo_nearest`` (include/scl_hip.h), for callers that size
things by them and for the tests.
"""
import numpy as np
import torch

from .. import _lib as L

_CHUNK = 1 << 22            # (query, reference) pairs per step of the NumPy functions: 32 MB of float64


def plan(r, q):
    """How ``scl_geo_nearest`` cuts an R x Q call: ``route`` ('refs': the lanes go over the
    references, Q <= ``_lib.GEO_SMALL_Q``; 'queries': one query per lane, ``_lib.GEO_BLOCK_QUERIES``
    per workgroup), ``slab`` (references per LDS slab), ``slabs_per_split``, ``split_rows``
    (references per split), ``splits`` and ``pairs``: the workspace is ``round256(8 pairs) +
    round256(4 pairs)`` bytes for ``pairs = min(Q slabs, max(Q, GEO_TARGET_BLOCKS GEO_BLOCK_QUERIES))``,
    a bound on ``Q splits`` that grows with Q and with R."""
    r, q = int(r), int(q)
    if r < 1 or q < 1:
        raise ValueError('plan: R and Q must be at least 1, got R=%d Q=%d' % (r, q))
    small = q <= L.GEO_SMALL_Q
    qblocks = q if small else -(-q // L.GEO_BLOCK_QUERIES)
    slabs = -(-r // L.GEO_SLAB)
    want = max(1, L.GEO_TARGET_BLOCKS // qblocks)
    per = -(-slabs // want)
    return {'route': 'refs' if small else 'queries', 'slab': L.GEO_SLAB, 'slabs_per_split': per,
            'split_rows': per * L.GEO_SLAB, 'splits': -(-slabs // per),
            'pairs': min(q * slabs, max(q, L.GEO_TARGET_BLOCKS * L.GEO_BLOCK_QUERIES))}


def _host_xy(a, name):
    """A host array as float64 [., 2], finite."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError('%s %s must be [., 2] with at least one row' % (name, a.shape))
    if not np.isfinite(a).all():
        raise ValueError('%s holds positions that are not finite' % name)
    return np.ascontiguousarray(a)


def _device_of(tensors, device):
    for t in tensors:
        if isinstance(t, torch.Tensor):
            return t.device
    return torch.device(device)


def _xy(dev, **named):
    """Every operand as float64 [., 2] dense on ``dev``: a host array is checked (all of them, before
    anything goes up) and uploaded, a tensor is taken as it is (a CPU tensor raises: there is no
    CPU fallback)."""
    checked = []
    for name, a in named.items():
        if isinstance(a, torch.Tensor):
            L.require_device(a)
            if a.dim() != 2 or a.shape[1] != 2 or a.shape[0] < 1:
                raise ValueError('%s %s must be [., 2] with at least one row' % (name, tuple(a.shape)))
            if a.device != dev:
                raise ValueError('%s is on %s, the call runs on %s' % (name, a.device, dev))
            checked.append(a)
        else:
            checked.append(_host_xy(a, name))
    return [a.to(torch.float64).contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(dev)
            for a in checked]


def _require_hip(dev):
    if dev.type != 'cuda':
        raise L.SclError('evaluation.geo needs a HIP device (nearest_np / hit_distances_np are the host '
                         'statement of the contract; no CPU fallback exists); got %r' % (dev,))


def nearest(ref_xy, query_xy, device='cuda'):
    """ref_xy [R, 2], query_xy [Q, 2] -> (idx int64 [Q], dist float64 [Q]) device tensors, on the
    current stream.  NumPy inputs are uploaded as float64 (to the device of the other operand, or
    ``device``)."""
    dev = _device_of((ref_xy, query_xy), device)
    _require_hip(dev)
    ref, qry = _xy(dev, ref_xy=ref_xy, query_xy=query_xy)
    lib = L.load()
    r, q = ref.shape[0], qry.shape[0]
    idx = torch.empty(q, dtype=torch.int64, device=dev)
    dist = torch.empty(q, dtype=torch.float64, device=dev)
    ws = L.workspace(lib.scl_geo_nearest_workspace_bytes(r, q), dev)
    with torch.cuda.device(dev):
        L.check(lib.scl_geo_nearest(L.ptr(ref), r, L.ptr(qry), q, L.ptr(idx), L.ptr(dist), L.ptr(ws),
                                    ws.numel(), L.stream_of(ref)))
    return idx, dist


def hit_distances(ref_xy, query_xy, idx, device='cuda'):
    """idx [Q, n] (any integer type, host or device: a retrieval call's hit list) ->
    float64 [Q, n] device tensor, on the current stream."""
    dev = _device_of((ref_xy, query_xy, idx), device)
    _require_hip(dev)
    ref, qry = _xy(dev, ref_xy=ref_xy, query_xy=query_xy)
    if isinstance(idx, torch.Tensor):
        L.require_device(idx)
        if idx.is_floating_point() or idx.device != dev:
            raise ValueError('idx must be an integer tensor on %s, got %s on %s' % (dev, idx.dtype, idx.device))
        hits = idx.to(torch.int64).contiguous()
    else:
        hits = np.asarray(idx)
        if hits.dtype.kind not in 'iu':
            raise ValueError('idx must hold integers, got %s' % (hits.dtype,))
        hits = torch.from_numpy(np.ascontiguousarray(hits, dtype=np.int64)).to(dev)
    q = qry.shape[0]
    if hits.dim() != 2 or hits.shape[0] != q or hits.shape[1] < 1:
        raise ValueError('idx %s must be [%d, n] with n >= 1' % (tuple(hits.shape), q))
    n = hits.shape[1]
    out = torch.empty((q, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().scl_geo_hit_dist(L.ptr(ref), ref.shape[0], L.ptr(qry), q, L.ptr(hits), n,
                                          L.ptr(out), L.stream_of(ref)))
    return out


def _d2(ref, qry):
    """[q, R] float64: NumPy rounds every operation on its own."""
    dx = ref[None, :, 0] - qry[:, None, 0]
    dy = ref[None, :, 1] - qry[:, None, 1]
    return dx * dx + dy * dy


def nearest_np(ref_xy, query_xy):
    """The definition of ``nearest`` in NumPy, ``_CHUNK`` pairs at a time."""
    ref = np.asarray(ref_xy, dtype=np.float64)
    qry = np.asarray(query_xy, dtype=np.float64)
    r, q = len(ref), len(qry)
    idx = np.empty(q, dtype=np.int64)
    dist = np.empty(q, dtype=np.float64)
    step = max(1, _CHUNK // max(r, 1))
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, q, step):
            d2 = _d2(ref, qry[s:s + step])
            nan = np.isnan(d2)
            d2[nan] = np.inf                               # a NaN never wins ...
            j = np.argmin(d2, axis=1)                      # (the first of equal values: the lower row)
            best = d2[np.arange(len(j)), j]
            none = nan.all(axis=1)                         # ... so where every d2 is NaN nothing does
            # +inf can win, but only over nothing: then the first row whose d2 is not NaN has it
            late = np.isinf(best) & ~none
            if late.any():
                j[late] = np.argmax(~nan[late], axis=1)
            idx[s:s + step] = np.where(none, -1, j)
            dist[s:s + step] = np.sqrt(best)
    return idx, dist


def hit_distances_np(ref_xy, query_xy, idx):
    """The definition of ``hit_distances`` in NumPy, ``_CHUNK`` pairs at a time."""
    ref = np.asarray(ref_xy, dtype=np.float64)
    qry = np.asarray(query_xy, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    q, n = idx.shape
    out = np.empty((q, n), dtype=np.float64)
    step = max(1, _CHUNK // max(n, 1))
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, q, step):
            hit = idx[s:s + step]
            valid = (hit >= 0) & (hit < len(ref))
            at = ref[np.where(valid, hit, 0)]                                  # [q, n, 2]
            dx = at[..., 0] - qry[s:s + step, None, 0]
            dy = at[..., 1] - qry[s:s + step, None, 1]
            out[s:s + step] = np.where(valid, np.sqrt(dx * dx + dy * dy), np.inf)
    return out

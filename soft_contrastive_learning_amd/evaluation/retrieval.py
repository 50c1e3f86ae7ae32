"""Exact L2 top-n retrieval, the replacement for the KDTree query of
``evaluation/top-n.py:103-108`` (also ``train/train.py:1181-1182``).

``topn_l2`` runs csrc/topn.hip on one device; ``RetrievalIndex`` prepares a fixed reference set
once and answers many small queries against it; ``merge_topn`` combines per-shard results
when the reference set is split over ranks (shard the reference set,
replicate the queries, all-gather the [Q,n] candidates, merge).
"""
import torch

from .. import _lib as L

MAX_N = 25          # what ONE kernel pass returns per query (32 nominated, 25 certified: csrc/topn.hip)


SCORE_MODES = {'f32': L.TOPN_SCORE_F32, 'bf16x3': L.TOPN_SCORE_BF16X3}


_WIDTHS = (32, 64, 128, 256)      # descriptor widths the kernels of csrc/topn.hip take
WIDE_MAX = 32768                  # columns of the widest row scl_topn_wide_query takes (a multiple of 256 from 512 on)


def _pad_width(t, width=None):
    """Rows zero-padded to ``width`` (default: the next one in ``_WIDTHS``); no distance changes."""
    width = width or next(c for c in _WIDTHS if t.shape[1] <= c)
    return t if t.shape[1] == width else torch.nn.functional.pad(t, (0, width - t.shape[1]))


def _checked(ref, query, n, width=None):
    """(ref, query) as contiguous float32 [R,d] / [Q,d] on a HIP device, with n in [1, R].
    ``width``: of the rows a RetrievalIndex was given (its ``ref`` is those rows, padded)."""
    L.require_device(ref, query)
    query = query.float().contiguous()
    if width is not None and (query.dim() != 2 or query.shape[1] != width):
        raise ValueError("query %s must be [Q,%d]" % (tuple(query.shape), width))
    if width is None:
        ref = ref.float().contiguous()
        if ref.dim() != 2 or query.dim() != 2 or ref.shape[1] != query.shape[1]:
            raise ValueError("ref %s / query %s must be [R,d] / [Q,d]" % (tuple(ref.shape), tuple(query.shape)))
    if n > ref.shape[0] or n < 1:
        raise ValueError("n must be in [1, R], got n=%d R=%d" % (n, ref.shape[0]))
    return ref, query


def _sized(nbytes, r, q, d, n, hint=''):
    if nbytes == 0:
        raise ValueError("unsupported retrieval shape R=%d Q=%d d=%d n=%d%s" % (r, q, d, n, hint))
    return nbytes


def _run(ref, query, n, idx_offset, certify, stats, call, window=None):
    """One kernel pass over ``ref`` [R, d], n <= MAX_N: pads the query to d, allocates the outputs,
    has ``call(query, idx, dist, flag, bound, count)`` make the C call(s) (flag, bound: None without
    ``certify``) and resolves exactly the queries that the call could not certify.  ``window`` =
    (positions, near, radius): the call is a windowed one and fills ``count`` (else None), which
    ``stats`` receives."""
    query = _pad_width(query, ref.shape[1])
    q, dev = query.shape[0], ref.device
    idx = torch.empty((q, n), dtype=torch.int64, device=dev)
    dist = torch.empty((q, n), dtype=torch.float64, device=dev)
    count = torch.empty(q, dtype=torch.int32, device=dev) if window is not None else None
    flag = torch.empty(q, dtype=torch.uint8, device=dev) if certify else None
    bound = torch.empty(q, dtype=torch.float64, device=dev) if certify else None
    call(query, idx, dist, flag, bound, count)
    if stats is not None and window is not None:
        stats['count'] = count
    if certify:
        bad = torch.nonzero(flag).reshape(-1)                      # (synchronises; usually empty)
        if stats is not None:
            stats['uncertified'] = int(bad.numel())
        if bad.numel():
            _resolve_exactly(ref, query, n, int(idx_offset), bad, bound, dist, idx, window=window)
    return dist, idx


def topn_l2(ref, query, n, idx_offset=0, score='f32', certify=True, stats=None):
    """ref [R,d], query [Q,d] float32 on a HIP device -> (dists [Q,n] float64 ascending,
    idx [Q,n] int64), like ``KDTree(ref).query(query, k=n, sort_results=True)``.

    ``score`` picks how the 32 candidates per (query, reference split) are nominated before
    the float64 re-rank: 'f32' (exact-float32 matrix instructions, score error ~1e-7) or
    'bf16x3' (three bf16 matrix products of the high/low operand halves: |score error| <=
    1.2e-5 |q||r|, about 1.8x faster).  The emitted distances are float64-exact either way.

    ``certify`` (default): the kernel proves per query that no reference outside the
    nominated 32 can reach the n-th exact distance (``scl_topn_l2_cert``); the queries it
    cannot prove this for — near-duplicate references around the n-th neighbour — are
    resolved by an exact float64 pass over every reference (``scl_topn_exact_filter``), so the
    index lists are exact with no assumption on the data.  ``stats`` (a dict) receives
    ``uncertified`` = how many queries took that path.  Descriptors wider than 256 take
    ``_topn_wide`` (nomination from the inner products of ``scl_topn_dots``, its own certificate
    of the same kind; ``score`` does not apply there)."""
    lib = L.load()
    if score not in SCORE_MODES:
        raise ValueError("score must be one of %s, got %r" % (sorted(SCORE_MODES), score))
    ref, query = _checked(ref, query, n)
    r, d = ref.shape
    if d > 256:
        return _topn_wide(ref, query, n, idx_offset, certify, stats)
    if n > MAX_N:
        # evaluation/top-n.py:135 leaves --N free; one kernel pass certifies 25 per query
        return _topn_many(ref, query, n, idx_offset, score, stats)
    ref = _pad_width(ref)
    d, flags = ref.shape[1], SCORE_MODES[score]

    def call(query, idx, dist, flag, bound, _):
        q = query.shape[0]
        nbytes = _sized(lib.scl_topn_l2_ex_workspace_bytes(r, q, d, n, flags), r, q, d, n,
                        " (d in {32,64,128,256}, n <= %d, n <= R)" % MAX_N)
        ws = L.workspace(nbytes, ref.device)
        L.check(lib.scl_topn_l2_cert(L.ptr(ref), r, L.ptr(query), q, d, n, int(idx_offset), L.ptr(idx),
                                     L.ptr(dist), L.ptr(flag), L.ptr(bound), L.ptr(ws), ws.numel(),
                                     flags, L.stream_of(ref)))
    return _run(ref, query, n, idx_offset, certify, stats, call)


class RetrievalIndex:
    """A fixed reference set prepared once for many ``topn_l2`` calls (a localiser: frames arrive
    one or a few at a time).  ``RetrievalIndex(ref, idx_offset, score).query(query, n, certify,
    stats)`` returns what ``topn_l2(ref, query, n, idx_offset, score, certify, stats)`` returns, in
    both tensors, for any data.

    Built once (``scl_topn_index_build``): the reference norms, their maximum and, with
    ``score='bf16x3'``, the two bf16 planes — what ``topn_l2`` recomputes per call.  A query of at
    most ``_lib.TOPN_STREAM_MAX_Q`` rows takes the stream route of ``scl_topn_index_query`` (one pass
    over the float32 rows on every CU); more rows run the scan of ``topn_l2`` from the index.
    ``stats`` also receives ``route``: 'stream', 'scan', or 'delegate' for what the index does not
    cover (descriptors wider than 256, n > 25: ``topn_l2`` on the stored rows).  A width that is not
    32, 64, 128 or 256 is zero-padded, once here and per query.  The index block and the workspace
    are tensors owned by the object; use one object per stream.

    ``positions`` [R, 2] (any float type, host or device; kept as float64) gives every reference a
    place on the ground and lets ``query(.., near=, radius=)`` restrict each query to the references
    within ``radius`` of its centre — a localiser's position prior.  With ``W_q = {j : radius_q >= 0
    and dx*dx + dy*dy <= radius_q*radius_q}`` (float64, every operation rounded on its own, as NumPy
    evaluates that expression; a negative or NaN radius: empty), row q of the answer is
    ``topn_l2(ref[W_q], query[q:q+1], min(n, |W_q|), 0, score)`` with its indices mapped back to the
    rows of ``ref`` (+ ``idx_offset``), filled up to n columns with index -1 (no offset) and distance
    +inf.  ``stats`` then receives ``route='window'``, ``count`` (int32 tensor [Q]: min(n, |W_q|))
    and ``uncertified``.  The call (``scl_topn_index_query_window``, 32 queries at a time) skips
    every 32-reference tile that no query's circle reaches, so on a traverse it costs what the
    windows cover.

    ``wide`` says what happens to descriptors wider than 256 columns.  'delegate' (default): nothing
    is prepared, every query is ``topn_l2`` on the stored rows and a window raises.  'resident'
    (``score='f32'``, at most ``WIDE_MAX`` columns): the rows are zero-padded to a multiple of 256
    once and the wide index block is built (``scl_topn_wide_index_build``: float64-summed norms and
    their bound); a query of at most ``_lib.TOPN_STREAM_MAX_Q`` rows and n <= 25 is then one
    ``scl_topn_wide_query`` (``route`` 'wide'), and windowed queries run the same call in groups
    (``route`` 'window').  The queries it cannot certify are resolved by ``_brute_force_f64``.  More
    rows or a larger n delegate as before.  At 256 columns or fewer ``wide`` changes nothing."""

    def __init__(self, ref, idx_offset=0, score='f32', positions=None, wide='delegate'):
        if score not in SCORE_MODES:
            raise ValueError("score must be one of %s, got %r" % (sorted(SCORE_MODES), score))
        if wide not in ('delegate', 'resident'):
            raise ValueError("wide must be 'delegate' or 'resident', got %r" % (wide,))
        L.require_device(ref)
        ref = ref.float().contiguous()
        if ref.dim() != 2 or ref.shape[0] < 1:
            raise ValueError("ref %s must be [R,d] with R >= 1" % (tuple(ref.shape),))
        self.idx_offset = int(idx_offset)
        self.score = score
        self.width = ref.shape[1]                      # of the rows as given
        self._flags = SCORE_MODES[score]
        self._ws = None
        self._index = None
        self._geo = None
        self._wide = False                             # the index block is the wide one
        self.positions = None
        if positions is not None:
            xy = torch.as_tensor(positions).to(ref.device, torch.float64).contiguous()
            if xy.dim() != 2 or tuple(xy.shape) != (ref.shape[0], 2):
                raise ValueError("positions %s must be [%d,2]" % (tuple(xy.shape), ref.shape[0]))
            self.positions = xy
        if self.width > 256 and wide == 'delegate':
            self.ref = ref                             # (topn_l2's wide path; nothing to prepare)
            return
        lib = L.load()
        if self.width > 256:
            if score != 'f32':
                raise ValueError("wide='resident' scores in float32: score must be 'f32', got %r" % (score,))
            if self.width > WIDE_MAX:
                raise ValueError("wide='resident' takes at most %d columns, got %d" % (WIDE_MAX, self.width))
            self.ref = ref = _pad_width(ref, -(-self.width // 256) * 256)
            self._wide = True
            r, d = ref.shape
            self._index = L.workspace(_sized(lib.scl_topn_wide_index_bytes(r, d), r, 1, d, 1), ref.device)
            L.check(lib.scl_topn_wide_index_build(L.ptr(ref), r, d, L.ptr(self._index), self._index.numel(),
                                                  L.stream_of(ref)))
            self._build_geo(lib)
            return
        self.ref = ref = _pad_width(ref)
        r, d = ref.shape
        nbytes = lib.scl_topn_index_bytes(r, d, self._flags)
        if nbytes == 0:
            raise ValueError("unsupported index shape R=%d d=%d" % (r, d))
        self._index = L.workspace(nbytes, ref.device)
        L.check(lib.scl_topn_index_build(L.ptr(ref), r, d, L.ptr(self._index), self._index.numel(),
                                         self._flags, L.stream_of(ref)))
        self._build_geo(lib)

    def _build_geo(self, lib):
        if self.positions is not None:
            r = self.ref.shape[0]
            self._geo = L.workspace(lib.scl_topn_geo_bytes(r), self.ref.device)
            L.check(lib.scl_topn_geo_build(L.ptr(self.positions), r, L.ptr(self._geo), self._geo.numel(),
                                           L.stream_of(self.ref)))

    def query(self, query, n, certify=True, stats=None, near=None, radius=None):
        """query [Q, width] float32 on the index's device -> (dist [Q,n] float64, idx [Q,n] int64).
        ``near`` [Q, 2] with ``radius`` (a scalar or [Q]): among the references of each query's window."""
        ref, query = _checked(self.ref, query, n, self.width)
        if near is not None or radius is not None:
            return self._query_window(query, n, certify, stats, near, radius)
        if self._index is None or n > MAX_N or (self._wide and query.shape[0] > L.TOPN_STREAM_MAX_Q):
            if stats is not None:
                stats['route'] = 'delegate'
            return topn_l2(ref[:, :self.width], query, n, self.idx_offset, self.score, certify, stats)
        lib = L.load()
        r, d = ref.shape

        def call(query, idx, dist, flag, bound, _):
            q = query.shape[0]
            self._workspace(lib.scl_topn_wide_query_workspace_bytes(r, q, d, n) if self._wide else
                            lib.scl_topn_index_query_workspace_bytes(r, q, d, n, self._flags), q, n)
            if stats is not None:
                stats['route'] = 'wide' if self._wide else 'stream' if q <= L.TOPN_STREAM_MAX_Q else 'scan'
            head = (L.ptr(ref), r, d, L.ptr(self._index), self._index.numel())
            out = (n, self.idx_offset, L.ptr(idx), L.ptr(dist))
            tail = (L.ptr(flag), L.ptr(bound), L.ptr(self._ws), self._ws.numel())
            if self._wide:
                L.check(lib.scl_topn_wide_query(*head, None, 0, L.ptr(query), q, None, None, *out, None, *tail,
                                                L.stream_of(ref)))
            else:
                L.check(lib.scl_topn_index_query(*head, L.ptr(query), q, *out, *tail, self._flags,
                                                 L.stream_of(ref)))
        return _run(ref, query, n, self.idx_offset, certify, stats, call)

    def _workspace(self, nbytes, q, n):
        """the object's workspace, grown to ``nbytes`` (0: a shape the library does not take)"""
        if nbytes == 0:
            _sized(0, self.ref.shape[0], q, self.ref.shape[1], n)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = L.workspace(nbytes, self.ref.device)

    def nearest_position(self, query_xy):
        """query_xy [Q, 2] (NumPy or a tensor on the index's device) -> (row int64 [Q], dist float64
        [Q]): the reference whose position is nearest each query's and its distance
        (``geo.nearest`` on the positions the index was built with: ties to the lower row; rows of
        ``ref``, + ``idx_offset``)."""
        from . import geo
        if self.positions is None:
            raise ValueError("nearest_position needs an index built with positions")
        row, dist = geo.nearest(self.positions, query_xy)
        if self.idx_offset:
            row = torch.where(row >= 0, row + self.idx_offset, row)
        return row, dist

    def hit_distances(self, query_xy, idx):
        """query_xy [Q, 2], idx [Q, n] as ``query`` returns it -> float64 [Q, n]: the distance on the
        ground between each query and each of its hits (``geo.hit_distances``); +inf for the -1 a
        windowed query pads with."""
        from . import geo
        if self.positions is None:
            raise ValueError("hit_distances needs an index built with positions")
        if self.idx_offset:
            idx = torch.as_tensor(idx).to(self.positions.device)
            idx = torch.where(idx >= 0, idx - self.idx_offset, idx)
        return geo.hit_distances(self.positions, query_xy, idx)

    def _query_window(self, query, n, certify, stats, near, radius):
        """``query`` with windows: ``scl_topn_index_query_window`` on groups of at most
        ``_lib.TOPN_STREAM_MAX_Q`` queries, then the exact resolution of the flagged ones."""
        ref = self.ref
        q, dev = query.shape[0], ref.device
        if near is None or radius is None:
            raise ValueError("a window needs both near and radius")
        if self.positions is None:
            raise ValueError("near/radius need an index built with positions")
        if self._geo is None or n > MAX_N:
            raise ValueError("a windowed query takes descriptors of at most 256 columns (wider ones with "
                             "wide='resident') and n <= %d, got width %d, n=%d" % (MAX_N, self.width, n))
        near = torch.as_tensor(near).to(dev, torch.float64).contiguous()
        if tuple(near.shape) != (q, 2):
            raise ValueError("near %s must be [%d,2]" % (tuple(near.shape), q))
        radius = torch.as_tensor(radius).to(dev, torch.float64)
        if radius.dim() == 0:
            radius = radius.expand(q)
        if tuple(radius.shape) != (q,):
            raise ValueError("radius %s must be a scalar or [%d]" % (tuple(radius.shape), q))
        radius = radius.contiguous()
        lib = L.load()
        r, d = ref.shape
        step = L.TOPN_STREAM_MAX_Q

        def call(query, idx, dist, flag, bound, count):
            for s in range(0, q, step):
                g = min(step, q - s)
                self._workspace(lib.scl_topn_wide_query_workspace_bytes(r, g, d, n) if self._wide else
                                lib.scl_topn_index_query_window_workspace_bytes(r, g, d, n, self._flags), g, n)
                part = slice(s, s + g)
                head = (L.ptr(ref), r, d, L.ptr(self._index), self._index.numel(), L.ptr(self._geo),
                        self._geo.numel(), L.ptr(query[part]), g, L.ptr(near[part]), L.ptr(radius[part]), n,
                        self.idx_offset, L.ptr(idx[part]), L.ptr(dist[part]), L.ptr(count[part]),
                        None if flag is None else L.ptr(flag[part]),
                        None if bound is None else L.ptr(bound[part]), L.ptr(self._ws), self._ws.numel())
                if self._wide:
                    L.check(lib.scl_topn_wide_query(*head, L.stream_of(ref)))
                else:
                    L.check(lib.scl_topn_index_query_window(*head, self._flags, L.stream_of(ref)))
            if stats is not None:
                stats['route'] = 'window'
        return _run(ref, query, n, self.idx_offset, certify, stats, call, (self.positions, near, radius))


_FILTER_CAP = 2048      # candidates within the bound kept per uncertified query


def _in_window(xy, cx, cy, rad):
    """The window's predicate on float64 tensors that broadcast: every operation rounded on its own."""
    dx, dy = xy[..., 0] - cx, xy[..., 1] - cy
    return (rad >= 0) & (dx * dx + dy * dy <= rad * rad)


def _resolve_exactly(ref, query, n, idx_offset, bad, bound, dist, idx, window=None):
    """Rows ``bad`` of (dist, idx) recomputed from the exact float64 distances to every
    reference that lies within the query's bound.  ``window`` = (positions, near, radius): among
    the references inside each query's window only (a flagged query's window holds at least n
    within its bound: the bound is the n-th distance of nominated MEMBERS).  Rows wider than the
    filter kernel takes (256 columns) go through ``_brute_force_f64`` one query at a time."""
    r, d = ref.shape
    if d > 256:
        for qi in bad.tolist():
            rows = None
            if window is not None:
                xy, near, radius = window
                rows = torch.nonzero(_in_window(xy, near[qi, 0], near[qi, 1], radius[qi])).reshape(-1)
            best_d, best_i = _brute_force_f64(ref if rows is None else ref[rows], query[qi], n)
            k = best_i.numel()                               # (a flagged query's window holds >= n)
            dist[qi, :k] = best_d.sqrt()
            idx[qi, :k] = (best_i if rows is None else rows[best_i]) + idx_offset
        return
    lib = L.load()
    dev = ref.device
    for s in range(0, bad.numel(), 4096):
        ql = bad[s:s + 4096].to(torch.int32).contiguous()
        nq = ql.numel()
        count = torch.empty(nq, dtype=torch.int32, device=dev)
        cd = torch.full((nq, _FILTER_CAP), float('inf'), dtype=torch.float64, device=dev)
        ci = torch.full((nq, _FILTER_CAP), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        L.check(lib.scl_topn_exact_filter(L.ptr(ref), r, L.ptr(query), d, L.ptr(ql), nq,
                                          L.ptr(bound), _FILTER_CAP, L.ptr(count), L.ptr(cd),
                                          L.ptr(ci), L.stream_of(ref)))
        if window is not None:
            xy, near, radius = window
            rows = ql.long()
            stored = ci < 2 ** 31 - 1
            inside = _in_window(xy[ci.clamp(max=r - 1).long()], near[rows, 0:1], near[rows, 1:2],
                                radius[rows, None]) & stored
            cd = cd.masked_fill(~inside, float('inf'))
            ci = ci.masked_fill(~inside, 2 ** 31 - 1)
        # order by (distance, index): stable sort by index first, then by distance
        o = torch.argsort(ci, dim=1, stable=True)
        cd, ci = torch.gather(cd, 1, o), torch.gather(ci, 1, o)
        o = torch.argsort(cd, dim=1, stable=True)[:, :n]
        rows = ql.long()
        dist[rows] = torch.gather(cd, 1, o).sqrt()
        idx[rows] = torch.gather(ci, 1, o).long() + idx_offset
        over = torch.nonzero(count > _FILTER_CAP).reshape(-1)
        for k in over.tolist():
            # more than _FILTER_CAP references within the n-th distance (thousands of exact
            # duplicates): plain float64 brute force for that query, in reference chunks
            qi = int(ql[k])
            if window is not None:
                # (a flagged query: at least n members)
                member = torch.nonzero(_in_window(xy, near[qi, 0], near[qi, 1], radius[qi])).reshape(-1)
                best_d, best_i = _brute_force_f64(ref[member], query[qi], n)
                best_i = member[best_i]
            else:
                best_d, best_i = _brute_force_f64(ref, query[qi], n)
            dist[qi] = best_d.sqrt()
            idx[qi] = best_i + idx_offset


def _topn_many(ref, query, n, idx_offset=0, score='f32', stats=None):
    """Exact top-n for n > 25 (``KDTree.query(k=N)`` with the reference's free ``--N``,
    evaluation/top-n.py:103-108, 135) from the exact, certified top-25 primitive.

    The references are dealt into S interleaved shards (``ref[s::S]``: neighbours that are
    adjacent in list order — consecutive frames of a traverse — spread over all shards); every
    shard returns its exact top-25 per query; the merged pool, ordered by (distance, index), gives
    the candidate n-th distance D_n.  A shard whose 25th distance is STRICTLY beyond D_n cannot
    hold anything else within D_n, so its contribution is complete.  For the (query, shard) pairs
    where that fails — more than 25 of the query's n nearest fell into one shard, or ties at D_n —
    the shard is split in two and those queries alone are asked again, until every pair is
    certified (a shard of <= 25 references returns all of them).  Exact for any data; the expected
    case (S chosen so that a shard holds ~n/S << 25 of the top n) is one pass and no refinement.
    ``stats['refined']`` counts the (query, shard) pairs that needed a split."""
    dev = ref.device
    r = ref.shape[0]
    q = query.shape[0]
    shards = max(2, -(-n // 10))                      # expected share of the top n per shard: <= 10
    inf = float('inf')
    pool_d = torch.full((q, 0), inf, dtype=torch.float64, device=dev)
    pool_i = torch.zeros((q, 0), dtype=torch.int64, device=dev)
    refined = 0
    # work list: (reference rows of the shard as a LongTensor of positions, query rows or None = all)
    work = [(torch.arange(s, r, shards, device=dev), None) for s in range(shards)]
    passes = []                                      # (positions, query rows, dists, local idx)
    while work:
        pos, qrows = work.pop()
        sub = ref[pos].contiguous()
        qq = query if qrows is None else query[qrows].contiguous()
        k = min(MAX_N, sub.shape[0])
        dd, ii = topn_l2(sub, qq, k, 0, score)
        passes.append((pos, qrows, dd, pos[ii]))
        # fold into the pool: rows of the asked queries only
        rows = torch.arange(q, device=dev) if qrows is None else qrows
        add_d = torch.full((q, k), inf, dtype=torch.float64, device=dev)
        add_i = torch.full((q, k), 2 ** 62, dtype=torch.int64, device=dev)
        add_d[rows], add_i[rows] = dd, pos[ii]
        pool_d, pool_i = torch.cat([pool_d, add_d], 1), torch.cat([pool_i, add_i], 1)
        if work:
            continue
        # every outstanding pass is in: merge by (distance, index), drop what a refined shard
        # returned a second time (same index: its parent already gave it), then the candidate
        # n-th distance per query and the test
        o = torch.argsort(pool_i, dim=1, stable=True)
        pd, pi = torch.gather(pool_d, 1, o), torch.gather(pool_i, 1, o)
        dup = torch.zeros_like(pi, dtype=torch.bool)
        dup[:, 1:] = pi[:, 1:] == pi[:, :-1]
        pd = pd.masked_fill(dup, inf)
        o = torch.argsort(pd, dim=1, stable=True)
        pd, pi = torch.gather(pd, 1, o), torch.gather(pi, 1, o)
        keep = min(pd.shape[1], 4 * n)
        pool_d, pool_i = pd[:, :keep].contiguous(), pi[:, :keep].contiguous()
        d_n = pool_d[:, n - 1]
        for pos, qrows, dd, _ in passes:
            if pos.numel() <= MAX_N:
                continue                              # the shard returned all it has
            rows = torch.arange(q, device=dev) if qrows is None else qrows
            bad = rows[~(dd[:, -1] > d_n[rows])]
            if bad.numel():
                refined += int(bad.numel())
                work.append((pos[0::2], bad))
                work.append((pos[1::2], bad))
        passes = []
    if stats is not None:
        stats['refined'] = refined
    return pool_d[:, :n].contiguous(), (pool_i[:, :n] + int(idx_offset)).contiguous()


_KEEP = 32          # candidates nominated per query before the exact re-rank (wide path: >= n + 8)


def _brute_force_f64(ref, qv, n, chunk=65536):
    """Exact float64 sum((q - r)^2) of one query against every reference, best n by
    (distance, index): the arithmetic of the tree the reference builds."""
    dev = ref.device
    qv = qv.double()
    best_d = torch.empty(0, dtype=torch.float64, device=dev)
    best_i = torch.empty(0, dtype=torch.int64, device=dev)
    step = max(1, min(chunk, (1 << 25) // max(ref.shape[1], 1)))       # <= 256 MB of float64
    for a in range(0, ref.shape[0], step):
        dd = ((ref[a:a + step].double() - qv) ** 2).sum(1)
        ii = torch.arange(a, a + dd.numel(), device=dev)
        best_d, best_i = torch.cat([best_d, dd]), torch.cat([best_i, ii])
        o2 = torch.argsort(best_d, stable=True)[:n]          # index-ascending input: ties by index
        best_d, best_i = best_d[o2], best_i[o2]
    return best_d, best_i


def _topn_wide(ref, query, n, idx_offset, certify=True, stats=None, dots_fn=None):
    """Descriptors wider than 256 (the in-training localisation check runs the KDTree on the
    raw 32768-d vectors, train/train.py:1181-1182; evaluation/top-n.py sweeps d up to 4096).

    Nomination: s(q, r) = |q|^2 + |r|^2 - 2 q.r with the inner products from the library's own
    kernel ``scl_topn_dots`` (csrc/topn.hip: float32 matrix instructions inside chunks of 256
    features, float64 across chunks; round 3 used the float64 library GEMM here), norms in
    float64, blocks of queries x references, the best 32 per query kept across blocks.  Those 32
    are re-ranked with the direct float64 sum((q - r)^2) — the tree's arithmetic — and ordered
    by (distance, index).

    Certificate (no assumption on the data): every reference OUTSIDE the nominated set has
    s >= tau (the largest nominated score), and |s - D| <= eps for the exact squared distance D,
    with eps = 2 [2 gamma |q| R_max + (d + 8) 2^-53 (|q| + R_max)^2]: gamma = 256 u / (1 - 256 u),
    u = 2^-24, bounds a 256-long float32 FMA chain in ANY order, chunks combine by Cauchy-Schwarz
    (so the bound does not grow with d), the second term covers the float64 chunk sums, the two
    norms and the final additions, and the leading 2 is safety.  So if the n-th exact distance
    among the nominated is strictly below tau - eps (inflated by the direct form's own
    2 (d + 2) 2^-53 relative error), no outsider can reach it.  Queries that fail the test — near
    duplicates around the n-th neighbour within eps (6e-5 in squared distance for unit
    descriptors), or more than 32 references that close — are resolved by ``_brute_force_f64``
    over every reference.  ``stats['uncertified']`` counts them.

    ``dots_fn(ref_block, query_block) -> [Q, R] float64`` replaces the HIP kernel in the CPU
    tests of the logic around it (tests/test_retrieval_wide.py: the same chunked arithmetic in
    NumPy); the product path has no such argument and no CPU fallback."""
    lib = L.load() if dots_fn is None else None
    r, d = ref.shape
    q = query.shape[0]
    dev = ref.device
    keep = max(_KEEP, n + 8)                  # n > 25 (evaluation/top-n.py:135): nominate more
    u = 2.0 ** -53
    g32 = 256.0 * 2.0 ** -24 / (1.0 - 256.0 * 2.0 ** -24)
    qb_max = 512
    rb = 8192
    out_d = torch.empty((q, n), dtype=torch.float64, device=dev)
    out_i = torch.empty((q, n), dtype=torch.int64, device=dev)
    sb = max(256, (1 << 27) // d)                             # <= 1 GB of float64 per norm block
    rn_all = torch.cat([(ref[a:a + sb].double() ** 2).sum(1) for a in range(0, r, sb)])
    r_max = float(rn_all.max().sqrt())
    uncertified = 0
    # feature-axis splits: enough grid layers to put a workgroup on every CU for small blocks
    chunks = -(-d // 256)
    tiles = -(-min(q, qb_max) // 64) * -(-min(r, rb) // 64)
    splits = max(1, min(chunks, 16, 512 // max(tiles, 1)))
    while splits > 1 and (splits - 1) * -(-chunks // splits) >= chunks:
        splits -= 1
    dots = torch.empty(splits * min(q, qb_max) * min(r, rb), dtype=torch.float64, device=dev)
    for qs in range(0, q, qb_max):
        qblk = query[qs:qs + qb_max]
        qb = qblk.shape[0]
        qn = torch.cat([(qblk[a:a + sb].double() ** 2).sum(1) for a in range(0, qb, sb)])
        cand_s, cand_i = [], []
        for rs in range(0, r, rb):
            rblk = ref[rs:rs + rb]
            nr = rblk.shape[0]
            if dots_fn is None:
                dv = dots[:splits * qb * nr].view(splits, qb, nr)
                L.check(lib.scl_topn_dots(L.ptr(rblk), nr, L.ptr(qblk), qb, d, splits, L.ptr(dv),
                                          L.stream_of(ref)))
                dv = dv.sum(0) if splits > 1 else dv[0]
            else:
                dv = dots_fn(rblk, qblk)
            sc = qn[:, None] + rn_all[None, rs:rs + nr] - 2.0 * dv
            k = min(keep, nr)
            sv, iv = torch.topk(sc, k, dim=1, largest=False)
            cand_s.append(sv)
            cand_i.append(iv + rs)
        sv, iv = torch.cat(cand_s, 1), torch.cat(cand_i, 1)
        k = min(keep, sv.shape[1])
        top_s, pick = torch.topk(sv, k, dim=1, largest=False)
        cand = torch.gather(iv, 1, pick)                                  # [qb, k]
        exact = torch.empty((qb, k), dtype=torch.float64, device=dev)
        step = max(1, (1 << 25) // (k * d))                               # <= 256 MB of float64
        for a in range(0, qb, step):
            diff = qblk[a:a + step].double()[:, None, :] - ref[cand[a:a + step]].double()
            exact[a:a + step] = (diff * diff).sum(-1)
        # order by (distance, index): stable sort by index first, then by distance
        o = torch.argsort(cand, dim=1, stable=True)
        exact, cand = torch.gather(exact, 1, o), torch.gather(cand, 1, o)
        o = torch.argsort(exact, dim=1, stable=True)[:, :n]
        dn = torch.gather(exact, 1, o)
        out_d[qs:qs + qb] = dn.sqrt()
        out_i[qs:qs + qb] = torch.gather(cand, 1, o) + int(idx_offset)
        if certify and r > k:                    # (r <= keep: every reference was re-ranked)
            tau = top_s.max(dim=1).values
            qnorm = qn.sqrt()
            eps = 2.0 * (2.0 * g32 * qnorm * r_max + (d + 8) * u * (qnorm + r_max) ** 2)
            ok = dn[:, n - 1] * (1.0 + 2.0 * (d + 2) * u) < tau - eps
            for qi in torch.nonzero(~ok).reshape(-1).tolist():
                bd, bi = _brute_force_f64(ref, query[qs + qi], n)
                out_d[qs + qi] = bd.sqrt()
                out_i[qs + qi] = bi + int(idx_offset)
                uncertified += 1
    if stats is not None:
        stats['uncertified'] = uncertified if certify else None
    return out_d, out_i


def merge_topn(dists, idxs, n):
    """Merge per-shard (dists, idx) lists into the global top-n, ordered by
    (distance, index) like the single-device kernel."""
    d = torch.cat(list(dists), dim=1)
    i = torch.cat(list(idxs), dim=1)
    # stable two-key sort: by index first, then (stably) by distance
    o = torch.argsort(i, dim=1, stable=True)
    d, i = torch.gather(d, 1, o), torch.gather(i, 1, o)
    o = torch.argsort(d, dim=1, stable=True)[:, :n]
    return torch.gather(d, 1, o), torch.gather(i, 1, o)

"""GPU checks of retrieval with a position prior (csrc/topn.hip: scl_topn_geo_build /
scl_topn_index_query_window, evaluation/retrieval.RetrievalIndex.query(near=, radius=)) and of the
localiser and the command on top of it (evaluation/localize.py).

The defining property: with W_q the references whose position satisfies, in NumPy float64,
``dx*dx + dy*dy <= radius*radius``, row q of the answer is ``retrieval.topn_l2(ref[W_q],
query[q:q+1], min(n, |W_q|))`` mapped back to the rows of ``ref`` and filled with (-1, inf), in
both tensors, bit for bit (both sides end in the same float64 re-rank arithmetic).  So that the
exact fallback cannot hide a broken scan, no query may need it where no near-duplicate is planted:
on these random sets the un-windowed route certifies every query, and a subset is only sparser."""
import re

import numpy as np
import pytest
import torch

from oracle import topn_np as TN
from tests import util_data as U
from tests.util_guard import FILL, Guarded as _Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _window(xy, centre, radius):
    """The specification's predicate, in NumPy float64."""
    dx, dy = xy[:, 0] - centre[0], xy[:, 1] - centre[1]
    with np.errstate(invalid='ignore'):
        return np.nonzero((radius >= 0) & (dx * dx + dy * dy <= radius * radius))[0]


def _expected(dev, ref, qry, xy, near, radius, n, idx_offset=0, kdtree=False):
    """(dist [Q,n], idx [Q,n], count [Q]) from ``retrieval.topn_l2`` on each query's gathered subset."""
    from soft_contrastive_learning_amd.evaluation import retrieval
    q = len(qry)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    dist = torch.full((q, n), float('inf'), dtype=torch.float64, device=dev)
    idx = torch.full((q, n), -1, dtype=torch.int64, device=dev)
    count = np.zeros(q, np.int32)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (q,))
    for k in range(q):
        w = _window(xy, near[k], radius[k])
        m = count[k] = min(n, len(w))
        if m == 0:
            continue
        wt = torch.tensor(w, device=dev)
        dd, ii = retrieval.topn_l2(rt[wt].contiguous(), qt[k:k + 1], m, 0, 'f32')
        dist[k, :m], idx[k, :m] = dd[0], wt[ii[0]] + idx_offset
        if kdtree:
            kd, ki = TN.topn_kdtree(ref[w], qry[k:k + 1], m)
            np.testing.assert_array_equal(w[ki[0]], wt[ii[0]].cpu().numpy())
            np.testing.assert_allclose(dd[0].cpu().numpy(), kd[0], rtol=1e-12, atol=0)
    return dist, idx, count


def _index(dev, ref, xy, idx_offset=0):
    from soft_contrastive_learning_amd.evaluation import retrieval
    return retrieval.RetrievalIndex(torch.tensor(ref, device=dev), idx_offset, 'f32', positions=xy)


def _assert_window_result(got, stats, want, certified=True):
    (got_d, got_i), (want_d, want_i, want_c) = got, want
    assert stats['route'] == 'window'
    np.testing.assert_array_equal(stats['count'].cpu().numpy(), want_c)
    assert stats['count'].dtype == torch.int32
    assert torch.equal(got_i, want_i), (got_i, want_i)
    assert torch.equal(got_d, want_d)
    if certified:
        assert stats['uncertified'] == 0, stats


def _traverse(r):
    j = np.arange(r, dtype=np.float64)
    return np.stack([620000.25 + j, 5735000.5 + 0.5 * np.sin(j / 50.0)], 1)


# ---- 1. a window that holds everything is no window -------------------------------------------------------
@pytest.mark.parametrize("r,q,d,n", [(33, 1, 32, 25), (4099, 32, 256, 25), (40000, 8, 128, 7),
                                     (65, 3, 64, 5)])
def test_window_of_everything_equals_the_unwindowed_query(dev, r, q, d, n):
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    index = _index(dev, ref, xy)
    qt = torch.tensor(qry, device=dev)
    st, sw = {}, {}
    want_d, want_i = index.query(qt, n, stats=st)
    got_d, got_i = index.query(qt, n, stats=sw, near=np.tile(xy[r // 2], (q, 1)), radius=1e12)
    assert st['route'] == 'stream' and sw['route'] == 'window'
    assert torch.equal(got_i, want_i) and torch.equal(got_d, want_d)
    assert sw['count'].tolist() == [n] * q
    assert sw['uncertified'] == 0 and st['uncertified'] == 0


# ---- 2./3. window sizes around every threshold, on a traverse and with permuted positions -----------------
_SIZES = (0, 1, 24, 25, 26, 31, 32, 33, 200, 4099)
# rows that windows are centred on: a split boundary of stream_plan (4099 rows: splits of 1025), a
# 32-row tile boundary, both ends of the list (the last tile is ragged) and a row of no distinction
_CENTRES = (1025, 2050, 64, 4090, 3, 3007)


def _threshold_case():
    r, q = 4099, 32
    xy = _traverse(r)
    near, radius = np.empty((q, 2)), np.empty(q)
    for k in range(q):
        m, c = _SIZES[k % len(_SIZES)], _CENTRES[(k + k // len(_SIZES)) % len(_CENTRES)]
        near[k] = xy[c]
        if m == 0:
            near[k] += (0.5, 3.0)                                        # off the track
            radius[k] = 1.0
            continue
        dx, dy = xy[:, 0] - near[k, 0], xy[:, 1] - near[k, 1]
        rad = np.sqrt(np.sort(dx * dx + dy * dy)[m - 1])                 # the m-th nearest lies ON the circle
        while len(_window(xy, near[k], rad)) < m:
            rad = np.nextafter(rad, np.inf)
        radius[k] = rad
    sizes = [len(_window(xy, near[k], radius[k])) for k in range(q)]
    assert sizes == [_SIZES[k % len(_SIZES)] for k in range(q)], sizes
    return xy, near, radius


@pytest.mark.parametrize("permuted", [False, True], ids=['traverse', 'permuted'])
def test_window_sizes_around_every_threshold(dev, permuted):
    """Windows of 0 .. R rows with the boundary reference exactly on the circle, some across a tile
    boundary and some across a split boundary.  Permuted: the same circles over positions shuffled
    against the rows — every tile's box then covers the track, no tile can be skipped, and the
    answer is still the subset's (the skip is an optimisation, never a semantic).  A float32
    position store fails the traverse case: the northings do not fit."""
    r, q, d, n = 4099, 32, 64, 25
    ref, qry = U.retrieval_sets(r, q, d)
    xy, near, radius = _threshold_case()
    if permuted:
        xy = xy[np.random.default_rng(4).permutation(r)]
    want = _expected(dev, ref, qry, xy, near, radius, n, kdtree=not permuted)
    assert sorted(set(want[2].tolist())) == [0, 1, 24, 25]
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, want)
    gi, gd = got[1].cpu().numpy(), got[0].cpu().numpy()
    for k in range(q):
        c = want[2][k]
        assert (gi[k, c:] == -1).all() and np.isinf(gd[k, c:]).all() and (gi[k, :c] >= 0).all()
        assert set(gi[k, :c]) <= set(_window(xy, near[k], radius[k]))


# ---- 4. the boundary is inclusive and exact -------------------------------------------------------------
def test_boundary_is_inclusive_and_exact(dev):
    r, d, n = 200, 32, 5
    ref, qry = U.retrieval_sets(r, 6, d)
    rng = np.random.default_rng(8)
    xy = np.stack([rng.integers(2000, 3000, r), rng.integers(2000, 3000, r)], 1).astype(np.float64)
    c = np.array([100.0, 200.0])
    on = {10: (3, 4), 77: (-3, -4), 140: (4, -3), 199: (5, 0), 33: (0, 0)}   # 3-4-5: exactly on the circle
    for row, off in on.items():
        xy[row] = c + off
    xy[50] = c + (3, 4)
    xy[50, 1] = np.nextafter(xy[50, 1], np.inf)                          # one ulp beyond
    xy[120] = c + (-5, 0)
    xy[120, 0] = np.nextafter(xy[120, 0], -np.inf)
    xy[60] = xy[61] = (7.0, 9.0)                                         # two references on one spot
    near = np.array([c, c, xy[60], c, c, c])
    radius = np.array([5.0, np.nextafter(5.0, 0.0), 0.0, -1.0, np.nan, -0.0])
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, _expected(dev, ref, qry, xy, near, radius, n, kdtree=True))
    gi = got[1].cpu().numpy()
    assert sorted(gi[0]) == sorted(on)                                   # all five, none of the two beyond
    assert sorted(gi[1]) == [-1, -1, -1, -1, 33]                         # a radius one ulp short of 5
    assert sorted(gi[2]) == [-1, -1, -1, 60, 61]                         # radius 0: the spot itself
    assert (gi[3] == -1).all() and (gi[4] == -1).all()                   # negative, NaN: empty
    assert sorted(gi[5]) == [-1, -1, -1, -1, 33]                         # -0.0 is a radius of zero
    assert st['count'].tolist() == [5, 1, 2, 0, 0, 1]


# ---- 5. many workgroups ----------------------------------------------------------------------------------
def test_many_workgroups(dev):
    """100003 rows: every CU works, most tiles are skipped; windows of about 80 rows on a split
    boundary (splits of 3126 rows), on the last, ragged tile and on row 0."""
    r, q, d, n = 100003, 8, 128, 7
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    centres = [3126, 100002, 0, 6252, 99990, 50000, 31, 3125]
    near, radius = xy[centres], np.full(q, 40.0)
    radius[5] = 3000.5                                                   # and one of 6001 rows
    want = _expected(dev, ref, qry, xy, near, radius, n)
    sizes = [len(_window(xy, near[k], radius[k])) for k in range(q)]
    assert 79 <= sizes[0] <= 81 and 40 <= sizes[1] <= 41 and 40 <= sizes[2] <= 41 and sizes[5] >= 5999, sizes
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, want)


# ---- 6. near-duplicate clusters across the window's edge ------------------------------------------------
def test_near_duplicate_clusters_across_the_window_edge(dev):
    """The construction of test_gpu_retrieval_index.test_near_duplicate_clusters with clusters twice
    the size, every second row of each placed outside the window: inside it lie that test's 48 near
    duplicates of query 3 and 60 exact duplicates near query 7, so both are flagged and resolved by
    the exact pass — among the members only."""
    rng = np.random.default_rng(123)
    r, q, d, n = 6000, 40, 128, 25
    ref = rng.standard_normal((r, d)).astype(np.float32)
    qry = rng.standard_normal((q, d)).astype(np.float32)
    rows_a = rng.permutation(r)[:96]
    ref[rows_a] = qry[3] * (1.0 + 1e-6 * rng.standard_normal((96, 1)).astype(np.float32)) \
        + 1e-6 * rng.standard_normal((96, d)).astype(np.float32)
    rows_b = np.setdiff1d(rng.permutation(r)[:160], rows_a)[:120]
    ref[rows_b] = (qry[7] + 0.01 * rng.standard_normal(d)).astype(np.float32)
    qry = qry[:32]
    xy = rng.uniform(-50.0, 50.0, (r, 2))                                # everything within 71 m of the origin
    others = np.setdiff1d(rng.permutation(r)[:1500], np.concatenate([rows_a, rows_b]))
    outside = np.concatenate([np.sort(rows_a)[::2], np.sort(rows_b)[::2], others])
    xy[outside] += (400.0, 0.0)
    near, radius = np.zeros((32, 2)), 100.0
    want = _expected(dev, ref, qry, xy, near, radius, n)
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, want, certified=False)
    assert 2 <= st['uncertified'] <= 6, st
    gi = got[1].cpu().numpy()
    assert not np.isin(gi, outside).any()                                # no outside row in any list
    assert list(gi[7]) == np.setdiff1d(rows_b, outside)[:n].tolist()     # exact ties: ascending row
    assert np.isin(gi[3], np.setdiff1d(rows_a, outside)).all()


# ---- 7. exact ties and an index offset ------------------------------------------------------------------
def test_ties_and_offset(dev):
    ref, qry = U.retrieval_sets(300, 10, 64)
    ref[150] = ref[3]          # exact tie inside the window: lower index first
    ref[200] = ref[3]          # and one outside it
    qry[0] = ref[3]
    xy = _traverse(300)
    near, radius = np.tile(xy[100], (10, 1)), np.full(10, 97.5)          # rows 3 .. 197
    radius[9] = 1.5                                                      # rows 99, 100, 101 only
    st = {}
    got = _index(dev, ref, xy, 1000).query(torch.tensor(qry, device=dev), 5, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, _expected(dev, ref, qry, xy, near, radius, 5, idx_offset=1000))
    d, i = got
    assert i[0, :2].tolist() == [1003, 1150] and d[0, :2].tolist() == [0.0, 0.0]
    assert 1200 not in i[0].tolist()
    assert sorted(i[9].tolist()) == [-1, -1, 1099, 1100, 1101]           # -1 stays -1
    assert int(i[:9].min()) >= 1003 and int(i.max()) <= 1197


# ---- 8. no state between calls --------------------------------------------------------------------------
def test_no_state_between_calls(dev):
    r, q, d, n = 5000, 32, 128, 25
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    qt = torch.tensor(qry, device=dev)
    wins = [(xy[np.arange(q) * 150], np.full(q, 60.0)), (xy[4900 - np.arange(q) * 100], np.linspace(0.0, 40.0, q))]
    one = _index(dev, ref, xy)
    first = one.query(qt, n, near=wins[0][0], radius=wins[0][1])
    plain = one.query(qt, n)
    second = one.query(qt[:5], n, near=wins[1][0][:5], radius=wins[1][1][:5])
    third = one.query(qt, n, near=wins[1][0], radius=wins[1][1])
    for got, fresh in ((first, _index(dev, ref, xy).query(qt, n, near=wins[0][0], radius=wins[0][1])),
                       (plain, _index(dev, ref, xy).query(qt, n)),
                       (second, _index(dev, ref, xy).query(qt[:5], n, near=wins[1][0][:5], radius=wins[1][1][:5])),
                       (third, _index(dev, ref, xy).query(qt, n, near=wins[1][0], radius=wins[1][1]))):
        assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    assert torch.equal(third[1][:5], second[1])
    assert not torch.equal(first[1], plain[1])


def test_more_than_32_queries_go_in_groups(dev):
    r, q, d, n = 3000, 70, 32, 5
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    near, radius = xy[(np.arange(q) * 41) % r], np.linspace(0.0, 30.0, q)
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, _expected(dev, ref, qry, xy, near, radius, n))


def test_refusals(dev):
    from soft_contrastive_learning_amd.evaluation import retrieval
    ref, qry = U.retrieval_sets(100, 2, 32)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    xy = _traverse(100)
    near = xy[:2]
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt).query(qt, 5, near=near, radius=1.0)          # no positions
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt, positions=xy).query(qt, 30, near=near, radius=1.0)   # n > 25
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt, positions=xy).query(qt, 5, near=near)        # half a window
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt, positions=xy[:50])
    wide_r, wide_q = U.retrieval_sets(100, 2, 520)
    wide = retrieval.RetrievalIndex(torch.tensor(wide_r, device=dev), positions=xy)
    with pytest.raises(ValueError):
        wide.query(torch.tensor(wide_q, device=dev), 5, near=near, radius=1.0)    # wider than 256
    # positions in any float type, on the host or the device
    want = retrieval.RetrievalIndex(rt, positions=xy).query(qt, 5, near=near, radius=10.0)
    xy32 = np.stack([np.arange(100.0), np.zeros(100)], 1).astype(np.float32)
    a = retrieval.RetrievalIndex(rt, positions=torch.tensor(xy32, device=dev)).query(
        qt, 5, near=torch.tensor(xy32[:2]), radius=torch.tensor([10.0, 10.0], dtype=torch.float32))
    b = retrieval.RetrievalIndex(rt, positions=xy32.astype(np.float64)).query(qt, 5, near=xy32[:2].tolist(), radius=10)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert want[1].shape == a[1].shape


# ---- 9. the geo block, the workspace and the outputs between guard bands ----------------------------------
def _window_between_bands(dev, fill, r=32771, q=8, d=32, n=5):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    centres = np.array([0, 31, 32, 1025, 16385, 32770, 32739, 20000])
    near, radius = xy[centres], np.array([3.0, 40.0, 0.0, 100.0, -1.0, 50.0, 1.5, 1e9])
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    xt, ct, rad = (torch.tensor(a, device=dev) for a in (xy, near, radius))
    index = L.workspace(lib.scl_topn_index_bytes(r, d, 0), dev)
    L.check(lib.scl_topn_index_build(L.ptr(rt), r, d, L.ptr(index), index.numel(), 0, L.stream_of(rt)))
    geo = _Guarded(dev, lib.scl_topn_geo_bytes(r), fill)
    L.check(lib.scl_topn_geo_build(L.ptr(xt), r, L.ptr(geo.inner), geo.inner.numel(), L.stream_of(rt)))
    geo.assert_bands_intact()
    ws = _Guarded(dev, lib.scl_topn_index_query_window_workspace_bytes(r, q, d, n, 0), fill)
    # q * n * 8 = 320 bytes and q * 4 = 32 bytes of output between their own bands
    idx, dist, count = _Guarded(dev, q * n * 8, FILL), _Guarded(dev, q * n * 8, FILL), _Guarded(dev, q * 4, FILL)
    flag = torch.ones(q, dtype=torch.uint8, device=dev)
    bound = torch.full((q,), -1.0, dtype=torch.float64, device=dev)
    L.check(lib.scl_topn_index_query_window(
        L.ptr(rt), r, d, L.ptr(index), index.numel(), L.ptr(geo.inner), geo.inner.numel(), L.ptr(qt), q,
        L.ptr(ct), L.ptr(rad), n, 0, L.ptr(idx.inner), L.ptr(dist.inner), L.ptr(count.inner), L.ptr(flag),
        L.ptr(bound), L.ptr(ws.inner), ws.inner.numel(), 0, L.stream_of(rt)))
    for g in (geo, ws, idx, dist, count):
        g.assert_bands_intact()
    out = (idx.inner.view(torch.int64).view(q, n).clone(), dist.inner.view(torch.float64).view(q, n).clone(),
           count.inner.view(torch.int32).clone(), flag, bound)
    # every output element was written: none still holds the fill pattern
    pat = torch.full((8,), FILL, dtype=torch.uint8, device=dev)
    assert not bool((out[0] == pat.view(torch.int64)).any())
    assert not bool((out[1] == pat.view(torch.float64)).any())
    assert not bool((out[2] == pat[:4].view(torch.int32)).any())
    assert int(flag.sum()) == 0 and bool((bound >= 0).all())
    want_d, want_i, want_c = _expected(dev, ref, qry, xy, near, radius, n)
    assert torch.equal(out[0], want_i) and torch.equal(out[1], want_d)
    np.testing.assert_array_equal(out[2].cpu().numpy(), want_c)
    assert want_c.tolist() == [3, 5, 1, 5, 0, 5, 3, 5]
    return out


def test_geo_block_workspace_and_outputs_between_guard_bands(dev):
    a, b = _window_between_bands(dev, FILL), _window_between_bands(dev, 0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 10. the localiser ------------------------------------------------------------------------------------
def _track(m, q, seed=5):
    rng = np.random.default_rng(seed)
    ref_xy = np.stack([620000.25 + 0.5 * np.arange(m), 5735000.5 + 0.1 * rng.standard_normal(m)], 1)
    qry_xy = np.stack([620000.25 + rng.uniform(0, 0.5 * m, q), 5735000.5 + rng.standard_normal(q)], 1)
    return ref_xy, qry_xy


@pytest.mark.parametrize("l", [0.0, 5.0])
def test_locate_descriptors_with_a_window(dev, l):
    from soft_contrastive_learning_amd.evaluation import localize, retrieval
    m, q, n = 400, 37, 5
    ref_xy, qry_xy = _track(m, q)
    ref_f, qry_f = U.retrieval_sets(m, q, 64)
    loc = localize.Localizer(ref_f, ref_xy, n=n, l=l, device=dev)
    kept = np.asarray(loc.ref_idx)
    assert (len(kept) < m // 5) == (l > 0)
    radius = np.linspace(0.0, 12.0, q)
    radius[5], radius[6] = -1.0, 1e9
    idx, fd, xy = loc.locate_descriptors(qry_f, near=qry_xy, radius=radius)
    want_d, want_i, want_c = _expected(dev, ref_f[kept], qry_f, ref_xy[kept], qry_xy, radius, n)
    want_i = want_i.cpu().numpy()
    assert 0 in want_c and n in want_c and ((want_c > 0) & (want_c < n)).any()
    np.testing.assert_array_equal(idx, np.where(want_i >= 0, kept[np.maximum(want_i, 0)], -1))
    np.testing.assert_array_equal(fd, want_d.cpu().numpy())
    np.testing.assert_array_equal(xy, np.where((idx >= 0)[..., None], ref_xy[np.maximum(idx, 0)], np.nan))
    assert idx.dtype == np.int64 and fd.dtype == np.float64 and xy.shape == (q, n, 2)
    # without a window: what it returns today
    idx0, fd0, xy0 = loc.locate_descriptors(qry_f)
    dd, ii = retrieval.topn_l2(torch.tensor(ref_f[kept], device=dev), torch.tensor(qry_f, device=dev), n)
    np.testing.assert_array_equal(idx0, kept[ii.cpu().numpy()])
    np.testing.assert_array_equal(fd0, dd.cpu().numpy())
    np.testing.assert_array_equal(xy0, ref_xy[idx0])
    assert loc.uncertified == 0


# ---- 11. the command --------------------------------------------------------------------------------------
def test_command_with_a_prior(dev, tmp_path, capsys):
    """A traverse whose first 300 references lie 1 m apart and whose last 75 lie 4 m apart; the frames
    drive along it.  A window of 30 m holds 25 references on the first stretch only."""
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.util import io
    n, radius, batch = 25, 30.0, 2                                       # (two frames: at most 24 m)
    x = np.concatenate([np.arange(300.0), 300.0 + 4.0 * np.arange(75)])
    ref_xy = np.stack([620000.25 + x, 5735000.5 + 0.5 * np.sin(x / 50.0)], 1)
    ref_f, _ = U.retrieval_sets(len(x), 1, 64)
    rows = np.arange(2, len(x), 3)                                       # the frames: noisy copies of these rows
    qry_f = (ref_f[rows] + 0.05 * np.random.default_rng(3).standard_normal((len(rows), 64))).astype(np.float32)
    qry_xy = ref_xy[rows] + 0.25
    for name, f in (('ref', ref_f), ('query', qry_f), ('pca', ref_f)):
        io.save_pickle([row for row in f], str(tmp_path / ('set_%s.v1.pickle' % name)))
    for name, xy in (('ref', ref_xy), ('query', qry_xy)):
        io.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]],
                     'northing': [repr(float(v)) for v in xy[:, 1]]}, str(tmp_path / ('%s.csv' % name)))

    def run(out, *more):
        capsys.readouterr()
        path = localize.main(['--pca_lv_pickle', str(tmp_path / 'set_pca.v1.pickle'),
                              '--query_lv_pickle', str(tmp_path / 'set_query.v1.pickle'),
                              '--ref_lv_pickle', str(tmp_path / 'set_ref.v1.pickle'),
                              '--query_csv', str(tmp_path / 'query.csv'), '--ref_csv', str(tmp_path / 'ref.csv'),
                              '--N', str(n), '--out_root', str(tmp_path / out), '--L', '0', '--D', '0',
                              '--batch', str(batch), *more])
        return path, capsys.readouterr().out
    off, said = run('off')
    assert 'searched again' not in said
    huge, said = run('huge', '--prior_radius', '1e9')
    assert open(off, 'rb').read() == open(huge, 'rb').read()
    assert re.search(r'\b0 frames searched again', said)
    on, said = run('on', '--prior_radius', str(radius))
    top_i, free = np.asarray(io.load_pickle(on)[0]), np.asarray(io.load_pickle(off)[0])
    assert list(top_i[:, 0]) == list(rows)                               # it tracks
    again = 0
    for s in range(batch, len(rows), batch):
        prior = ref_xy[top_i[s - 1, 0]]
        inside = _window(ref_xy, prior, radius)
        for k in range(s, min(s + batch, len(rows))):
            if len(inside) < n:                                          # searched again, everywhere
                again += 1
                np.testing.assert_array_equal(top_i[k], free[k])
            else:                                                        # every hit within 30 m of the prior
                assert np.isin(top_i[k], inside).all(), k
    assert 0 < again < len(rows) - batch
    assert int(re.search(r'(\d+) frames searched again', said).group(1)) == again
    assert (top_i != free).any()

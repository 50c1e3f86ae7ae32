"""GPU checks of the geographic ground truth (csrc/geo_eval.hip: scl_geo_nearest / scl_geo_hit_dist;
evaluation/geo.py) and of the front ends' ``geo='device'`` route.

Every assertion on a kernel's output is EQUALITY of both tensors with ``geo.nearest_np`` /
``geo.hit_distances_np``, the NumPy statement of the contract: d2 = dx*dx + dy*dy in float64 with
every operation rounded on its own, the lexicographically smallest (d2, row), sqrt correctly
rounded, NaN never wins, +inf can, nothing -> (-1, inf).  The shapes are named from the granules the
Python layer exports (``_lib.GEO_*``, ``geo.plan``): slab, queries per workgroup, the small-Q
route and the rows per split."""
import os

import numpy as np
import pytest
import torch

from tests import util_data as U
from tests.geo_data import expanded_form_bound, golden_run
from tests.util_guard import FILL, Guarded

pytestmark = pytest.mark.gpu

R_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 100003)
Q_SIZES = (1, 2, 31, 32, 33, 64, 65, 257)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _utm(n, seed, spread=3.0):
    """A traverse at UTM magnitudes with steps of 0.2 .. `spread` m: full float64 fractions, so a
    float32 shortcut or a fused multiply-add changes bits."""
    rng = np.random.default_rng(seed)
    head = np.cumsum(rng.normal(0.0, 0.08, n))
    step = rng.uniform(0.2, spread, n)
    return np.array([620000.0, 5700000.0]) + np.cumsum(np.stack([step * np.cos(head), step * np.sin(head)], 1), 0)


def _queries(ref, q, seed):
    rng = np.random.default_rng(seed)
    return ref[rng.integers(0, len(ref), q)] + rng.normal(0.0, 2.0, (q, 2))


def _check(dev, ref, qry, hits=None):
    """Both calls on device tensors against the NumPy definition: equality, dtypes, shapes."""
    from soft_contrastive_learning_amd.evaluation import geo
    rt, qt = torch.from_numpy(ref).to(dev), torch.from_numpy(qry).to(dev)
    idx, dist = geo.nearest(rt, qt)
    want_i, want_d = geo.nearest_np(ref, qry)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float64 and idx.shape == dist.shape == (len(qry),)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(dist.cpu().numpy(), want_d)
    if hits is not None:
        got = geo.hit_distances(rt, qt, torch.from_numpy(hits).to(dev))
        assert got.dtype == torch.float64 and got.shape == hits.shape
        np.testing.assert_array_equal(got.cpu().numpy(), geo.hit_distances_np(ref, qry, hits))
    return want_i, want_d


@pytest.mark.parametrize('r', R_SIZES)
def test_shapes_in_traverse_order_and_permuted(dev, r):
    ref = _utm(r, seed=r)
    perm = np.random.default_rng(r + 1).permutation(r)
    for q in Q_SIZES:
        qry = _queries(ref, q, seed=7 * q)
        hits = np.random.default_rng(q).integers(0, r, (q, 5))
        want_i, _ = _check(dev, ref, qry, hits)
        if r > 5000 and q not in (2, 33, 257):
            continue
        got_i, _ = _check(dev, np.ascontiguousarray(ref[perm]), qry, hits)
        np.testing.assert_array_equal(perm[got_i], want_i)          # (no two rows of a traverse coincide)


def _granule_cases():
    """(R, Q) one below, at and one above every granule: the slab, the rows of a split where there is
    more than one slab per split, the queries of a workgroup, the small-Q route's limit."""
    from soft_contrastive_learning_amd import _lib as L
    from soft_contrastive_learning_amd.evaluation import geo
    cases = []
    for q in (1, L.GEO_SMALL_Q, L.GEO_SMALL_Q + 1, L.GEO_BLOCK_QUERIES + 1):
        # the least R at which this Q's splits take two slabs each, and around it
        qblocks = q if q <= L.GEO_SMALL_Q else -(-q // L.GEO_BLOCK_QUERIES)
        edge = (L.GEO_TARGET_BLOCKS // qblocks) * L.GEO_SLAB
        assert geo.plan(edge, q)['slabs_per_split'] == 1 and geo.plan(edge + 1, q)['slabs_per_split'] == 2
        rows = geo.plan(edge + 1, q)['split_rows']
        assert rows == 2 * L.GEO_SLAB
        cases += [(r, q) for r in (edge - 1, edge, edge + 1, edge + rows - 1, edge + rows, edge + rows + 1)]
    for q in (L.GEO_BLOCK_QUERIES - 1, L.GEO_BLOCK_QUERIES, L.GEO_BLOCK_QUERIES + 1, 2 * L.GEO_BLOCK_QUERIES,
              2 * L.GEO_BLOCK_QUERIES + 1):
        cases += [(3 * L.GEO_SLAB + 5, q)]
    return cases


@pytest.mark.parametrize('r,q', _granule_cases())
def test_one_below_at_and_one_above_every_granule(dev, r, q):
    ref = _utm(r, seed=3, spread=0.4)
    # queries next to the LAST rows and the rows around the first split boundary, so that a lost tail
    # or a lost boundary row changes an answer
    from soft_contrastive_learning_amd.evaluation import geo
    rows = geo.plan(r, q)['split_rows']
    targets = np.array([r - 1, r - 2, 0, min(rows, r - 1), min(rows, r - 1) - 1, r // 2])
    qry = ref[targets[np.arange(q) % len(targets)]] + np.random.default_rng(q).normal(0.0, 0.01, (q, 2))
    want_i, _ = _check(dev, ref, qry, np.stack([targets[:5]] * q) if q <= 33 else None)
    assert want_i[0] == r - 1


@pytest.mark.parametrize('q', [1, 40])
def test_ties_go_to_the_lower_row_across_lanes_waves_slabs_and_splits(dev, q):
    from soft_contrastive_learning_amd import _lib as L
    from soft_contrastive_learning_amd.evaluation import geo
    r = 5 * L.GEO_TARGET_BLOCKS * L.GEO_SLAB // 4 + 77         # more than one slab per split
    p = geo.plan(r, q)
    assert p['splits'] > 2 and p['route'] == ('refs' if q == 1 else 'queries')
    base = _utm(r, seed=11) + 5000.0                       # everything far from the planted point
    spot = np.array([620010.125, 5700020.375])
    qry = np.tile(spot + np.array([0.3, -0.4]), (q, 1))
    qry[1:] += np.random.default_rng(1).normal(0, 0.01, (q - 1, 2))
    # equal positions at rows in different lanes, waves, slabs (a lane's next turn) and splits
    rows = [r - 1, 2 * p['split_rows'] + 7, p['split_rows'] + 5, p['split_rows'], p['split_rows'] - 1,
            L.GEO_SLAB + 5, 5 + 64, 5 + 1, 5]
    ref = base.copy()
    for k, row in enumerate(rows):
        ref[row] = spot                                    # the lowest planted row so far is `row`
        want_i, want_d = _check(dev, ref, qry)
        assert (want_i == row).all() and (want_d > 0).all(), (k, row)
    # all references equal: row 0; the doubled row 0 of the thinning loop at l = 0
    want_i, _ = _check(dev, np.tile(spot, (r, 1)), qry)
    assert (want_i == 0).all()
    traverse = _utm(1000, seed=2)
    doubled = traverse[[0] + list(range(1000))]
    near0 = np.tile(traverse[0], (q, 1)) + 0.01
    want_i, _ = _check(dev, doubled, near0, np.zeros((q, 2), dtype=np.int64) + [0, 1])
    assert (want_i == 0).all()


@pytest.mark.parametrize('q', [1, 40])
def test_the_winner_is_decided_on_d2_not_on_its_root(dev, q):
    """(nextafter(3, 4), 4) and (3, 4) against (0, 0): d2 = 25 + 1 ulp and 25, both roots 5.0."""
    from soft_contrastive_learning_amd.evaluation import geo
    above, exact = [np.nextafter(3.0, 4.0), 4.0], [3.0, 4.0]
    r = 70000
    rows = geo.plan(r, q)['split_rows']
    qry = np.zeros((q, 2))
    for a, b in ((0, 1), (5, 5 + 64), (100, 100 + 256), (3, rows + 3), (rows - 1, rows), (7, r - 1), (r - 2, r - 1)):
        ref = np.full((r, 2), 1000.0) + np.arange(r)[:, None]
        ref[a], ref[b] = above, exact                      # the later row has the smaller d2
        want_i, want_d = _check(dev, ref, qry)
        assert (want_i == b).all() and (want_d == 5.0).all()
        ref[a], ref[b] = exact, above
        want_i, want_d = _check(dev, ref, qry)
        assert (want_i == a).all() and (want_d == 5.0).all()


@pytest.mark.parametrize('q', [1, 2, 40, 300])
def test_nan_never_wins_and_infinity_can(dev, q):
    r = 3000
    ref = _utm(r, seed=4)
    qry = _queries(ref, q, seed=5)
    clean_i, _ = _check(dev, ref, qry)
    holed = ref.copy()
    holed[r // 2] = np.nan                                  # a NaN reference in the middle
    holed[clean_i[0]] = [np.nan, ref[clean_i[0], 1]]        # ... and in place of query 0's winner
    holed[7, 1] = -np.nan
    want_i, want_d = _check(dev, holed, qry, np.array([[r // 2, 0, clean_i[0], 7]] * q))
    assert want_i[0] != clean_i[0] and (want_i >= 0).all() and np.isfinite(want_d).all()
    # all NaN: -1 / inf
    want_i, want_d = _check(dev, np.full((r, 2), np.nan), qry)
    assert (want_i == -1).all() and np.isinf(want_d).all()
    # a far reference whose d2 overflows to +inf still wins over nothing, the first of two
    far = np.full((r, 2), np.nan)
    far[1234], far[2000] = [1e200, 0.0], [-1e300, 1e300]
    want_i, want_d = _check(dev, far, qry)
    assert (want_i == 1234).all() and np.isinf(want_d).all()
    # ... and loses to anything finite, wherever that is
    far[2999] = [1e150, 0.0]
    want_i, want_d = _check(dev, far, qry)
    assert (want_i == 2999).all() and np.isfinite(want_d).all()
    # a NaN query
    qry2 = qry.copy()
    qry2[0, 0] = np.nan
    want_i, want_d = _check(dev, ref, qry2, np.array([[0, 1]] * q))
    assert want_i[0] == -1 and np.isinf(want_d[0])


@pytest.mark.parametrize('n', [1, 5, 25, 26])
def test_hit_distances_of_any_index_list(dev, n):
    r, q = 1000, 70
    ref = _utm(r, seed=8)
    qry = _queries(ref, q, seed=9)
    hits = np.random.default_rng(n).integers(0, r, (q, n))
    bad = np.array([-1, -5, r, r + 7, 2 ** 40, -2 ** 40, 2 ** 31, -2 ** 31 - 1, 2 ** 32 + 3, np.iinfo(np.int64).min,
                    np.iinfo(np.int64).max])
    flat = hits.reshape(-1)
    where = np.random.default_rng(n + 1).choice(flat.size, size=min(flat.size // 2, 4 * len(bad)), replace=False)
    flat[where] = bad[np.arange(len(where)) % len(bad)]                # ... between valid ones
    from soft_contrastive_learning_amd.evaluation import geo
    _check(dev, ref, qry, hits)
    got = geo.hit_distances(torch.from_numpy(ref).to(dev), qry, hits).cpu().numpy()       # host operands go up
    invalid = (hits < 0) | (hits >= r)
    assert np.isinf(got[invalid]).all() and np.isfinite(got[~invalid]).all() and invalid.any() and (~invalid).any()
    direct = np.sqrt(((ref[np.where(invalid, 0, hits)] - qry[:, None, :]) ** 2).sum(-1))
    np.testing.assert_array_equal(got[~invalid], direct[~invalid])


def test_hit_lists_of_the_retrieval_calls(dev):
    """An idx taken straight from topn_l2 and from a windowed RetrievalIndex.query with its padding;
    RetrievalIndex.nearest_position / hit_distances against the plain calls."""
    from soft_contrastive_learning_amd.evaluation import geo, retrieval
    r, q, n = 700, 37, 25
    ref_f, qry_f = U.retrieval_sets(r, q, 64)
    xy = _utm(r, seed=12)
    qxy = _queries(xy, q, seed=13)
    rt, qt = torch.tensor(ref_f, device=dev), torch.tensor(qry_f, device=dev)
    xt, qxt = torch.from_numpy(xy).to(dev), torch.from_numpy(qxy).to(dev)
    _, idx = retrieval.topn_l2(rt, qt, n)
    got = geo.hit_distances(xt, qxt, idx)
    np.testing.assert_array_equal(got.cpu().numpy(), geo.hit_distances_np(xy, qxy, idx.cpu().numpy()))
    index = retrieval.RetrievalIndex(rt, 0, 'f32', positions=xy)
    stats = {}
    _, widx = index.query(qt[:32], n, near=qxy[:32], radius=10.0, stats=stats)
    count = stats['count'].cpu().numpy()
    assert (count < n).any() and (count > 0).any() and bool((widx == -1).any())          # padded rows exist
    got = index.hit_distances(qxt[:32], widx).cpu().numpy()
    np.testing.assert_array_equal(got, geo.hit_distances_np(xy, qxy[:32], widx.cpu().numpy()))
    assert np.isinf(got[widx.cpu().numpy() < 0]).all() and (got[widx.cpu().numpy() >= 0] <= 10.0).all()
    assert torch.equal(index.hit_distances(qxy[:32], widx), geo.hit_distances(xt, qxt[:32], widx))
    for a, b in zip(index.nearest_position(qxy), geo.nearest(xt, qxt)):
        assert torch.equal(a, b)
    want_i, want_d = geo.nearest_np(xy, qxy)
    np.testing.assert_array_equal(index.nearest_position(qxt)[0].cpu().numpy(), want_i)
    np.testing.assert_array_equal(index.nearest_position(qxt)[1].cpu().numpy(), want_d)
    # an index offset moves the rows and nothing else; no positions: both raise, like near=
    shifted = retrieval.RetrievalIndex(rt, 1000, 'f32', positions=xy)
    np.testing.assert_array_equal(shifted.nearest_position(qxy)[0].cpu().numpy(), want_i + 1000)
    _, sidx = shifted.query(qt[:32], n, near=qxy[:32], radius=10.0)
    assert torch.equal(shifted.hit_distances(qxy[:32], sidx), index.hit_distances(qxy[:32], widx))
    bare = retrieval.RetrievalIndex(rt, 0, 'f32')
    with pytest.raises(ValueError, match='positions'):
        bare.nearest_position(qxy)
    with pytest.raises(ValueError, match='positions'):
        bare.hit_distances(qxy, idx)


@pytest.mark.parametrize('r,q', [(1000, 1), (1000, 40), (70001, 32), (70001, 300)])
def test_guard_bands_stay_intact_and_nothing_is_read_before_it_is_written(dev, r, q):
    from soft_contrastive_learning_amd import _lib as L
    from soft_contrastive_learning_amd.evaluation import geo
    lib = L.load()
    ref = _utm(r, seed=21)
    qry = _queries(ref, q, seed=22)
    n = 5
    hits = np.random.default_rng(3).integers(-3, r + 3, (q, n))
    rt, qt, ht = torch.from_numpy(ref).to(dev), torch.from_numpy(qry).to(dev), torch.from_numpy(hits).to(dev)
    nbytes = lib.scl_geo_nearest_workspace_bytes(r, q)
    results = []
    for fill in (FILL, 0):
        ws = Guarded(dev, nbytes, fill)
        idx, dist, hd = Guarded(dev, 8 * q, fill), Guarded(dev, 8 * q, fill), Guarded(dev, 8 * q * n, fill)
        for _ in range(2):                                          # the second call finds the first one's leftovers
            L.check(lib.scl_geo_nearest(L.ptr(rt), r, L.ptr(qt), q, L.ptr(idx.inner), L.ptr(dist.inner),
                                        L.ptr(ws.inner), nbytes, L.stream_of(rt)))
            L.check(lib.scl_geo_hit_dist(L.ptr(rt), r, L.ptr(qt), q, L.ptr(ht), n, L.ptr(hd.inner), L.stream_of(rt)))
            for g in (ws, idx, dist, hd):
                g.assert_bands_intact()
            results.append((idx.inner.view(torch.int64).clone(), dist.inner.view(torch.float64).clone(),
                            hd.inner.view(torch.float64).clone()))
    want_i, want_d = geo.nearest_np(ref, qry)
    want_h = geo.hit_distances_np(ref, qry, hits).reshape(-1)
    for gi, gd, gh in results:                                      # two calls in a row, two fills: the same bits
        np.testing.assert_array_equal(gi.cpu().numpy(), want_i)
        np.testing.assert_array_equal(gd.cpu().numpy(), want_d)
        np.testing.assert_array_equal(gh.cpu().numpy(), want_h)


def test_two_streams_at_once_on_one_reference_set(dev):
    from soft_contrastive_learning_amd.evaluation import geo
    r = 100003
    ref = _utm(r, seed=31)
    rt = torch.from_numpy(ref).to(dev)
    sets = [(_queries(ref, q, seed=40 + q), torch.cuda.Stream(dev)) for q in (300, 7)]
    tens = [torch.from_numpy(qry).to(dev) for qry, _ in sets]
    torch.cuda.synchronize()
    out = []
    for rounds in range(3):
        for (qry, stream), qt in zip(sets, tens):
            with torch.cuda.stream(stream):
                idx, dist = geo.nearest(rt, qt)
                out.append((qry, idx, dist, geo.hit_distances(rt, qt, idx[:, None])))
    torch.cuda.synchronize()
    want = {id(qry): geo.nearest_np(ref, qry) for qry, _ in sets}
    for qry, idx, dist, hd in out:
        np.testing.assert_array_equal(idx.cpu().numpy(), want[id(qry)][0])
        np.testing.assert_array_equal(dist.cpu().numpy(), want[id(qry)][1])
        np.testing.assert_array_equal(hd.cpu().numpy()[:, 0], want[id(qry)][1])


# ---- the front ends -------------------------------------------------------------------------------

def _direct_table(qry_xy, ref_xy):
    dx = ref_xy[None, :, 0] - qry_xy[:, None, 0]
    dy = ref_xy[None, :, 1] - qry_xy[:, None, 1]
    return np.sqrt(dx * dx + dy * dy)


def _assert_payloads_identical(got, want):
    assert [type(v).__name__ for v in got] == [type(v).__name__ for v in want] \
        == ['list', 'list', 'ndarray', 'list', 'ndarray', 'list']
    assert got[0] == want[0] and got[3] == want[3] and got[5] == want[5]
    assert type(got[0][0]) is type(want[0][0]) is list and type(got[0][0][0]) is type(want[0][0][0]) is int
    assert type(got[1][0]) is type(want[1][0]) is list and type(got[1][0][0]) is type(want[1][0][0])
    assert type(got[3][0]) is type(want[3][0]) is int
    np.testing.assert_array_equal(np.asarray(got[1]), np.asarray(want[1]))
    for k in (2, 4):
        assert got[k].dtype == want[k].dtype == np.float64 and got[k].shape == want[k].shape
        np.testing.assert_array_equal(got[k], want[k])


@pytest.mark.parametrize('l', [0.0, 1.5])
def test_localizer_payload_from_positions_is_the_direct_form_tables(dev, l):
    from soft_contrastive_learning_amd.evaluation import localize
    ds = U.retrieval_dataset(n_pca=8, n_ref=400, n_query=50, e=64)
    loc = localize.Localizer(ds['ref_f'], ds['ref_xy'], n=5, l=l, device=dev)
    dist, local = loc.query_thinned(ds['query_f'])
    table = _direct_table(ds['query_xy'], ds['ref_xy'])
    _assert_payloads_identical(loc.payload(local, dist, query_xy=ds['query_xy']), loc.payload(local, dist, table))
    _assert_payloads_identical(localize.localize_set(loc, ds['query_f'], batch=7, query_xy=ds['query_xy']),
                               localize.localize_set(loc, ds['query_f'], table, batch=7))
    # padded hits (a window with fewer than n references) carry index -1 and distance inf
    dist, local = loc.query_thinned(ds['query_f'][:8], near=ds['query_xy'][:8], radius=3.0)
    assert (local < 0).any() and (local >= 0).any()
    top_i, top_g, top_f, gt_i, gt_g, ref_idx = loc.payload(local, dist, query_xy=ds['query_xy'][:8])
    top_i, top_g = np.asarray(top_i), np.asarray(top_g)
    assert (top_i[local < 0] == -1).all() and np.isinf(top_g[local < 0]).all() and np.isinf(top_f[local < 0]).all()
    np.testing.assert_array_equal(top_i[local >= 0], np.asarray(ref_idx)[local[local >= 0]])
    assert (top_g[local >= 0] <= 3.0 + 1e-9).all()
    want = loc.payload(np.where(local < 0, 0, local), dist, table[:8])
    np.testing.assert_array_equal(top_g[local >= 0], np.asarray(want[1])[local >= 0])
    assert gt_i == want[3] and np.array_equal(gt_g, want[4])


def _write_dataset(tmp_path, ds):
    from soft_contrastive_learning_amd.util import io as sio
    argv = []
    for name, xy in (('ref', ds['ref_xy']), ('query', ds['query_xy'])):
        path = str(tmp_path / ('set_%s.csv' % name))
        sio.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]], 'northing': [repr(float(v)) for v in xy[:, 1]]}, path)
        argv += ['--%s_csv' % name, path]
    for name in ('pca', 'ref', 'query'):
        path = str(tmp_path / ('set_%s.v1.pickle' % name))
        sio.save_pickle([row for row in ds[name + '_f']], path)
        argv += ['--%s_lv_pickle' % name, path]
    return argv


def _assert_device_pickle_matches_table_pickle(dev_path, table_path, ds, golden):
    """--geo device against --geo table: the retrieval's part and the types equal, gt_i the golden's,
    the geographic distances within the expanded form's own error (tests/test_geo_eval_host.py)."""
    from soft_contrastive_learning_amd.util import io as sio
    got, want = sio.load_pickle(dev_path), sio.load_pickle(table_path)
    assert [type(v).__name__ for v in got] == [type(v).__name__ for v in want] \
        == ['list', 'list', 'ndarray', 'list', 'ndarray', 'list']
    assert got[0] == want[0] and got[5] == want[5]                      # top_i, ref_idx
    np.testing.assert_array_equal(got[2], want[2])                      # top_f_dists
    assert type(got[0][0][0]) is type(want[0][0][0]) and type(got[1][0][0]) is type(want[1][0][0])
    assert type(got[3][0]) is type(want[3][0])
    assert got[3] == want[3] and np.array_equal(np.asarray(got[3]), golden['gt_i'])
    assert got[4].dtype == want[4].dtype == np.float64
    top_i = np.asarray(got[0])
    found = top_i >= 0
    for mine, table, ref_rows, qxy in (
            (got[4], want[4], ds['ref_xy'][np.asarray(got[3])], ds['query_xy']),
            (np.asarray(got[1]), np.asarray(want[1]), ds['ref_xy'][np.where(found, top_i, 0)], ds['query_xy'][:, None, :])):
        ok = np.isfinite(mine)
        assert np.array_equal(ok, np.isfinite(table))
        bound = expanded_form_bound(qxy, ref_rows, np.where(ok, mine, 0.0))
        err = np.abs(np.where(ok, table, 0.0) ** 2 - np.where(ok, mine, 0.0) ** 2)
        print('max |table^2 - device^2| / bound = %.3f' % (err / bound).max())
        assert (err <= bound).all()
    # ... and the device's numbers ARE the direct form
    direct = _direct_table(ds['query_xy'], ds['ref_xy'])
    np.testing.assert_array_equal(got[4], direct[np.arange(len(direct)), np.asarray(got[3])])
    np.testing.assert_array_equal(np.asarray(got[1])[found], np.take_along_axis(direct, np.where(found, top_i, 0), 1)[found])
    return got


def test_top_n_script_with_both_geo_routes(dev, tmp_path):
    from soft_contrastive_learning_amd.evaluation import top_n
    c, ds, golden = golden_run()
    files = _write_dataset(tmp_path, ds)
    out = {}
    for route in ('table', 'device'):
        argv = files + ['--N', str(c['N']), '--out_root', str(tmp_path / route), '--geo', route]
        written = top_n.main(argv)
        assert [os.path.relpath(w, str(tmp_path / route)) for w in written] == c['written']
        out[route] = written[0]
    _assert_device_pickle_matches_table_pickle(out['device'], out['table'], ds, golden)


@pytest.mark.parametrize('prior', [0.0, 100.0])
def test_localize_script_with_both_geo_routes(dev, tmp_path, prior):
    from soft_contrastive_learning_amd.evaluation import localize
    c, ds, golden = golden_run()
    files = _write_dataset(tmp_path, ds)
    out = {}
    for route in ('table', 'device'):
        argv = files + ['--N', str(c['N']), '--out_root', str(tmp_path / route), '--geo', route, '--batch', '8',
                        '--prior_radius', str(prior)]
        out[route] = localize.main(argv)
    got = _assert_device_pickle_matches_table_pickle(out['device'], out['table'], ds, golden)
    assert np.isfinite(np.asarray(got[1])).all() == (np.asarray(got[0]) >= 0).all()

"""Host-side checks of the geographic ground truth (no GPU): the C-ABI additions of
include/scl_hip.h (declared, exported, bound, the size query, validation before any launch), the
NumPy statement of the contract in evaluation/geo.py on hand cases and on the golden run of the
reference's evaluation/top-n.py, and the new options of the front ends."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.geo_data import expanded_form_bound, golden_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")
NEW = ("scl_geo_nearest_workspace_bytes", "scl_geo_nearest", "scl_geo_hit_dist")
NULL, SHAPE, WORKSPACE = -3, -1, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def _round256(n):
    return (n + 255) // 256 * 256


# ---- the C ABI ------------------------------------------------------------------------------------

def test_the_three_symbols_are_declared_exported_and_bound(lib):
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    diag = _lib.load(diag=True)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None and getattr(diag, name) is not None
    assert re.search(r"#define\s+SCL_ABI_VERSION\s+12\b", src)          # purely additive
    for macro, value in (('SCL_GEO_SLAB', _lib.GEO_SLAB), ('SCL_GEO_BLOCK_QUERIES', _lib.GEO_BLOCK_QUERIES),
                         ('SCL_GEO_SMALL_Q', _lib.GEO_SMALL_Q), ('SCL_GEO_TARGET_BLOCKS', _lib.GEO_TARGET_BLOCKS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro


def test_workspace_query_is_a_pure_host_function_and_follows_the_plan(lib):
    from soft_contrastive_learning_amd.evaluation import geo
    f = lib.scl_geo_nearest_workspace_bytes
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 5) == 0 and f(5, -3) == 0
    for r in (1, 255, 256, 257, 4097, 100000, 262144, 262145, 2 ** 31 - 1):
        last = 0
        for q in (1, 2, 3, 31, 32, 33, 256, 257, 512, 513, 1000, 10000, 262144, 262145, 10 ** 6):
            p = geo.plan(r, q)
            got = f(r, q)
            assert got == _round256(8 * p['pairs']) + _round256(4 * p['pairs']), (r, q)
            assert got % 256 == 0 and got > 0
            assert q * p['splits'] <= p['pairs']                                     # what the call writes fits
            assert p['split_rows'] == p['slabs_per_split'] * p['slab'] and p['slab'] == 256
            assert (p['splits'] - 1) * p['split_rows'] < r <= p['splits'] * p['split_rows']      # no empty split
            assert p['route'] == ('refs' if q <= 32 else 'queries')
            assert got >= last, (r, q)                                               # monotone in Q
            last = got
    for r in (200, 100000):
        sizes = [f(r, q) for q in range(1, 1200)]
        assert sizes == sorted(sizes)
        assert all(q * geo.plan(r, q)['splits'] <= geo.plan(r, q)['pairs'] for q in range(1, 1200))
    assert [f(r, 1000) for r in (1, 300, 5000, 100000, 10 ** 7)] == sorted(f(r, 1000) for r in (1, 300, 5000, 100000, 10 ** 7))
    # the benchmark shape: 10 000 queries, 40 query blocks, 25 splits of 16 slabs
    assert geo.plan(100000, 10000) == {'route': 'queries', 'slab': 256, 'slabs_per_split': 16,
                                       'split_rows': 4096, 'splits': 25, 'pairs': 262144}
    assert geo.plan(100000, 1)['splits'] == 391 and geo.plan(100000, 32)['splits'] == 31
    with pytest.raises(ValueError):
        geo.plan(0, 1)


def test_every_validation_code_comes_back_before_any_launch(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, a16, a8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 16), ctypes.c_void_p(base + 8)
    ws = lib.scl_geo_nearest_workspace_bytes(1000, 40)
    assert 0 < ws <= (1 << 16) - 512

    def nearest(ref=p, r=1000, qry=p, q=40, idx=p, dist=p, work=p, nbytes=ws):
        return lib.scl_geo_nearest(ref, r, qry, q, idx, dist, work, nbytes, None)

    def hits(ref=p, r=1000, qry=p, q=40, idx=p, n=5, dist=p):
        return lib.scl_geo_hit_dist(ref, r, qry, q, idx, n, dist, None)

    # NULL operands — before the shape
    for kw in (dict(ref=None), dict(qry=None), dict(idx=None), dict(dist=None), dict(work=None)):
        assert nearest(r=0, nbytes=0, **kw) == NULL, kw
    for kw in (dict(ref=None), dict(qry=None), dict(idx=None), dict(dist=None)):
        assert hits(q=0, **kw) == NULL, kw
    # shapes — before the workspace
    assert nearest(r=0, nbytes=0) == SHAPE and nearest(q=0, nbytes=0) == SHAPE
    assert nearest(r=-5, nbytes=0) == SHAPE and nearest(q=-1, nbytes=0) == SHAPE
    assert nearest(ref=a8, nbytes=0) == SHAPE and nearest(qry=a8, nbytes=0) == SHAPE    # 16-byte pairs
    assert hits(r=0) == SHAPE and hits(q=0) == SHAPE and hits(n=0) == SHAPE and hits(n=-2) == SHAPE
    assert hits(ref=a8) == SHAPE and hits(qry=a8) == SHAPE
    assert hits(q=2 ** 31 - 1, n=2 ** 31 - 1) == SHAPE                                   # Q n above 2^38
    # the workspace: one byte short, not 256-byte aligned
    assert nearest(nbytes=ws - 1) == WORKSPACE and nearest(nbytes=0) == WORKSPACE
    assert nearest(work=a16) == WORKSPACE and nearest(work=a8, nbytes=ws + 256) == WORKSPACE


# ---- the NumPy statement of the contract ----------------------------------------------------------

def test_numpy_definition_on_hand_cases():
    from soft_contrastive_learning_amd.evaluation.geo import hit_distances_np, nearest_np
    # 3-4-5, and a query on a reference
    ref = np.array([[10.0, 10.0], [3.0, 4.0], [-7.0, 1.0]])
    qry = np.array([[0.0, 0.0], [-7.0, 1.0]])
    idx, dist = nearest_np(ref, qry)
    assert idx.dtype == np.int64 and dist.dtype == np.float64
    assert idx.tolist() == [1, 2] and dist.tolist() == [5.0, 0.0]
    got = hit_distances_np(ref, qry, np.array([[1, 2, -1, 3], [2, 0, 1, -5]]))
    assert got.dtype == np.float64 and got.shape == (2, 4)
    assert got[0].tolist() == [5.0, np.sqrt(50.0), np.inf, np.inf]
    assert got[1].tolist() == [0.0, np.sqrt(17.0 * 17.0 + 81.0), np.sqrt(109.0), np.inf]
    # the tie goes to the lower row, wherever the equal rows are
    ref = np.array([[9.0, 9.0], [0.0, 2.0], [2.0, 0.0], [0.0, -2.0], [-2.0, 0.0]])
    assert nearest_np(ref, np.zeros((1, 2)))[0].tolist() == [1]
    assert nearest_np(ref[::-1], np.zeros((1, 2)))[0].tolist() == [0]
    # the doubled row 0 of the thinning loop at l = 0 (evaluation/top-n.py:91-94)
    xy = np.array([[1.0, 1.0], [5.0, 5.0], [9.0, 9.0]])
    doubled = xy[[0, 0, 1, 2]]
    idx, dist = nearest_np(doubled, np.array([[1.5, 1.0], [6.0, 5.0]]))
    assert idx.tolist() == [0, 2] and dist.tolist() == [0.5, 1.0]
    # NaN never wins, +inf can, nothing -> -1 / inf
    ref = np.array([[np.nan, 0.0], [1e200, 0.0], [np.nan, np.nan]])
    idx, dist = nearest_np(ref, np.zeros((1, 2)))
    assert idx.tolist() == [1] and dist.tolist() == [np.inf]
    idx, dist = nearest_np(ref[[0, 2]], np.zeros((2, 2)))
    assert idx.tolist() == [-1, -1] and dist.tolist() == [np.inf, np.inf]
    idx, dist = nearest_np(np.array([[np.nan, 0.0], [3.0, 4.0]]), np.zeros((1, 2)))
    assert idx.tolist() == [1] and dist.tolist() == [5.0]


def test_numpy_definition_is_chunked_over_the_queries(monkeypatch):
    from soft_contrastive_learning_amd.evaluation import geo
    rng = np.random.default_rng(3)
    ref = rng.uniform(-50, 50, (70, 2))
    qry = rng.uniform(-50, 50, (33, 2))
    hit = rng.integers(-2, 72, (33, 4))
    want = geo.nearest_np(ref, qry), geo.hit_distances_np(ref, qry, hit)
    monkeypatch.setattr(geo, '_CHUNK', 150)                     # two queries per step / 37 per step
    got = geo.nearest_np(ref, qry), geo.hit_distances_np(ref, qry, hit)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
    assert np.array_equal(got[1], want[1])
    d = np.sqrt(((ref[None] - qry[:, None]) ** 2).sum(-1))
    assert np.array_equal(want[0][0], d.argmin(1))


def test_the_winner_is_decided_on_d2_not_on_its_root():
    """Query (0, 0); reference 0 = (nextafter(3, 4), 4), reference 1 = (3, 4): their d2 differ
    (25 + 1 ulp against 25) and both roots are 5.0, so an argmin over ROOTS would take row 0."""
    from soft_contrastive_learning_amd.evaluation.geo import nearest_np
    ref = np.array([[np.nextafter(3.0, 4.0), 4.0], [3.0, 4.0]])
    d2 = ref[:, 0] * ref[:, 0] + ref[:, 1] * ref[:, 1]
    assert d2[1] == 25.0 and d2[0] == np.nextafter(25.0, 26.0)                 # the inputs' own property
    assert np.sqrt(d2[0]) == 5.0 and np.sqrt(d2[1]) == 5.0
    assert int(np.argmin(np.sqrt(d2))) == 0
    idx, dist = nearest_np(ref, np.zeros((1, 2)))
    assert idx.tolist() == [1] and dist.tolist() == [5.0]


def test_golden_ground_truth_within_the_expanded_forms_own_error():
    """On tests/util_data.retrieval_dataset the reference's own run (the golden fixture) and the
    direct form agree on the nearest reference of every query, and their distances differ by no
    more than the error of the table's EXPANDED form:

    scikit-learn's ``euclidean`` computes d2_table = (|q|^2 + (-2 q.r)) + |r|^2 in float64, clamped at
    0.  First-order count of its roundings, u = 2^-53: each norm is two squares and a sum, every one
    of the three rounded results at most the norm itself: <= 3 u |q|^2 and <= 3 u |r|^2; the inner
    product is two products and a sum, each at most |q||r| in magnitude: <= 3 u |q||r|, doubled
    (exactly) <= 6 u |q||r| <= 3 u (|q|^2 + |r|^2); the two additions round results no larger than
    |q|^2 + |r|^2 once each (the second, being d2 itself, far less): <= 2 u (|q|^2 + |r|^2).  Sum:
    |d2_table - d2| <= 8 u (|q|^2 + |r|^2), with d2 the exact value; clamping a negative result to 0
    only moves it towards d2 >= 0.  The direct form's own error against the exact value (three
    roundings relative to d2 itself, metres against 10^6 m) and the square root and squaring this
    test needs to compare stored DISTANCES (two roundings relative to d2 on each side) are covered
    by 8 u d2.  Observed maximum on this set: 0.16 of the bound (0.0188 m between the two forms)."""
    from soft_contrastive_learning_amd.evaluation import top_n
    from soft_contrastive_learning_amd.evaluation.geo import hit_distances_np, nearest_np
    c, ds, want = golden_run()
    ref_idx = top_n.thin_reference(ds['ref_xy'], c['l'])
    assert ref_idx[:2] == [0, 0]
    thinned = ds['ref_xy'][ref_idx]
    idx, dist = nearest_np(thinned, ds['query_xy'])
    gt_i = np.asarray(ref_idx)[idx]
    assert np.array_equal(gt_i, want['gt_i'])
    bound = expanded_form_bound(ds['query_xy'], ds['ref_xy'][gt_i], dist)
    err = np.abs(want['gt_g'] ** 2 - dist ** 2)
    print('gt_g_dist: max |table^2 - direct^2| / bound = %.3f, max |table - direct| = %.4g m'
          % ((err / bound).max(), np.abs(want['gt_g'] - dist).max()))
    assert (err <= bound).all()
    assert not np.array_equal(want['gt_g'], dist)                 # the two forms do differ
    # the hit distances of the reference run's own lists, the same way
    back = {orig: row for row, orig in reversed(list(enumerate(ref_idx)))}       # original -> lowest thinned row
    local = np.vectorize(back.get)(want['top_i'])
    hits = hit_distances_np(thinned, ds['query_xy'], local)
    bound = expanded_form_bound(ds['query_xy'][:, None, :], ds['ref_xy'][want['top_i']], hits)
    err = np.abs(want['top_g'] ** 2 - hits ** 2)
    print('top_g_dists: max |table^2 - direct^2| / bound = %.3f' % (err / bound).max())
    assert (err <= bound).all()


# ---- the front ends -------------------------------------------------------------------------------

def _numpy_topn(ref_f, query_f, n):
    d = np.sqrt(((query_f.astype(np.float64)[:, None, :] - ref_f.astype(np.float64)[None]) ** 2).sum(-1))
    i = np.argsort(d, axis=1, kind='stable')[:, :n]
    return np.take_along_axis(d, i, 1), i


def _track(m=60, q=9, e=8, seed=5):
    rng = np.random.default_rng(seed)
    ref_xy = np.stack([0.5 * np.arange(m), 0.1 * rng.standard_normal(m)], 1)
    qry_xy = np.stack([rng.uniform(0, 0.5 * m, q), rng.standard_normal(q)], 1)
    return ref_xy, qry_xy, rng.standard_normal((m, e)).astype(np.float32), rng.standard_normal((q, e)).astype(np.float32)


def test_device_calls_refuse_a_cpu_device_and_bad_host_input():
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.evaluation import geo
    ref, qry = np.zeros((4, 2)), np.ones((3, 2))
    with pytest.raises(_lib.SclError):
        geo.nearest(ref, qry, device='cpu')
    with pytest.raises(_lib.SclError):
        geo.nearest(torch.from_numpy(ref), torch.from_numpy(qry))
    with pytest.raises(_lib.SclError):
        geo.hit_distances(ref, qry, np.zeros((3, 2), dtype=np.int64), device='cpu')
    with pytest.raises(_lib.SclError):
        geo.hit_distances(torch.from_numpy(ref), qry, np.zeros((3, 2), dtype=np.int64))
    # host inputs are checked before anything goes up: finite, [., 2]
    bad = ref.copy()
    bad[2, 1] = np.nan
    for a, b in ((bad, qry), (ref, np.array([[np.inf, 0.0]])), (np.zeros((4, 3)), qry), (ref, np.zeros(2)),
                 (np.zeros((0, 2)), qry)):
        with pytest.raises(ValueError):
            geo.nearest(a, b)
        with pytest.raises(ValueError):
            geo.hit_distances(a, b, np.zeros((len(np.atleast_2d(b)), 1), dtype=np.int64))


def test_front_ends_take_the_option_and_refuse_what_it_cannot_do(tmp_path):
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.evaluation import localize, top_n
    ref_xy, qry_xy, ref_f, qry_f = _track()
    rt, qt = torch.from_numpy(ref_f), torch.from_numpy(qry_f)
    with pytest.raises(ValueError, match='full_query_xy'):
        top_n.retrieve(rt, qt, None, ref_xy, 5, 0.0, 'f32', geo='device')
    with pytest.raises(_lib.SclError):                                   # CPU tensors
        top_n.retrieve(rt, qt, None, ref_xy, 5, 0.0, 'f32', geo='device', full_query_xy=qry_xy)
    with pytest.raises(_lib.SclError):
        top_n.get_top_n(ref_f, ref_f, qry_f, ref_xy, qry_xy, n=5, d=4, device='cpu', geo='device')
    with pytest.raises(ValueError, match='geo'):
        top_n.retrieve(rt, qt, None, ref_xy, 5, 0.0, 'f32', geo='gpu')
    with pytest.raises(ValueError, match='geo'):
        top_n.get_top_n(ref_f, ref_f, qry_f, ref_xy, qry_xy, n=5, d=4, geo='host')
    # --geo parses in both commands, defaults to the table, and takes nothing else
    files = ['--pca_lv_pickle', 'p', '--query_lv_pickle', 'q', '--ref_lv_pickle', 'r', '--query_csv', 'qc',
             '--ref_csv', 'rc']
    for parser in (top_n.main_parser(), localize.main_parser()):
        assert parser.parse_args(files).geo == 'table'
        assert parser.parse_args(files + ['--geo', 'device']).geo == 'device'
        assert parser.parse_args(files + ['--geo', 'table']).geo == 'table'
        with pytest.raises(SystemExit):
            parser.parse_args(files + ['--geo', 'host'])
    # --geo device needs the resident index: with the CPU stand-in it raises, before any file is read
    with pytest.raises(ValueError, match='geo device'):
        localize.main(files + ['--geo', 'device', '--out_root', str(tmp_path)], query_fn=_numpy_topn)
    loc = localize.Localizer(ref_f, ref_xy, n=5, l=0.0, query_fn=_numpy_topn)
    d, i = loc.query_thinned(qry_f)
    with pytest.raises(ValueError, match='resident index'):
        loc.payload(i, d, query_xy=qry_xy)
    with pytest.raises(ValueError):
        loc.payload(i, d)
    with pytest.raises(ValueError):
        loc.payload(i, d, np.zeros((9, 60)), qry_xy)
    with pytest.raises(ValueError, match='resident index'):
        localize.localize_set(loc, qry_f, query_xy=qry_xy)

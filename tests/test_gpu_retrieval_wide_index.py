"""GPU checks of the resident index for descriptors wider than 256 columns (csrc/topn.hip:
scl_topn_wide_index_build / scl_topn_wide_query; evaluation/retrieval.RetrievalIndex(wide='resident'))
and of the localiser and the command on top of it.

The definition: un-windowed, row q is the exact top n of ``ref`` by float64 ``sum((q - r)**2)``,
ordered by (distance, index) — what ``retrieval.topn_l2`` returns: equal indices, distances within
``2 (d + 2) 2^-53`` relatively (both sides are float64 sums of the same d terms in different orders).
Windowed, the same against ``topn_l2`` on each query's gathered subset, filled with (-1, +inf), and
equal counts.  On integer-valued descriptors every sum is exact and both tensors are equal bit for
bit.  So that the exact fallback cannot hide a broken score kernel, no query may need it where no
near-duplicate is planted (``uncertified == 0``)."""
import re

import numpy as np
import pytest
import torch

from oracle import topn_np as TN
from tests import util_data as U
from tests.test_gpu_retrieval_window import _expected, _threshold_case, _traverse, _window
from tests.util_guard import FILL, Guarded as _Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rtol(d):
    return 2.0 * (d + 2) * 2.0 ** -53


def _close(got, want, d):
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy() if isinstance(want, torch.Tensor) else want,
                               rtol=_rtol(d), atol=0)


def _index(dev, ref, xy=None, idx_offset=0):
    from soft_contrastive_learning_amd.evaluation import retrieval
    return retrieval.RetrievalIndex(torch.tensor(ref, device=dev), idx_offset, 'f32', positions=xy,
                                    wide='resident')


# ---- 1. un-windowed: every width class, ragged tiles, one and many workgroups ---------------------------
@pytest.mark.parametrize("r,q,d,n", [
    (33, 1, 512, 25),
    (1000, 5, 512, 25),
    (4099, 32, 512, 25),        # ragged last tile, full query tile
    (4099, 32, 1024, 1),        # the whole query in LDS, at its limit
    (2050, 7, 520, 7),          # padded to 768
    (3000, 4, 2048, 25),        # two groups of chunks, re-staged per round
    (1500, 3, 4096, 25),        # the tightest certificate of the set
    (600, 2, 32768, 5),
    (40000, 2, 512, 25),        # more tiles than waves: several rounds
])
def test_unwindowed_is_the_exact_top_n(dev, r, q, d, n):
    from soft_contrastive_learning_amd.evaluation import retrieval
    ref, qry = U.retrieval_sets(r, q, d)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    st = {}
    got_d, got_i = _index(dev, ref).query(qt, n, stats=st)
    assert st['route'] == 'wide'
    kd_d, kd_i = TN.topn_kdtree(ref, qry, n)
    l2_d, l2_i = retrieval.topn_l2(rt, qt, n)
    np.testing.assert_array_equal(got_i.cpu().numpy(), kd_i)
    assert torch.equal(got_i, l2_i)
    _close(got_d, l2_d, d)
    _close(got_d, kd_d, d)
    assert got_d.dtype == torch.float64 and got_i.dtype == torch.int64 and tuple(got_i.shape) == (q, n)
    assert st['uncertified'] == 0, st


def test_what_the_route_does_not_cover_delegates_or_raises(dev):
    from soft_contrastive_learning_amd.evaluation import retrieval
    ref, qry = U.retrieval_sets(300, 40, 512)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    index = retrieval.RetrievalIndex(rt, wide='resident')
    for rows, n in ((qt, 5), (qt[:4], 30)):                              # more than 32 queries; n > 25
        st = {}
        got = index.query(rows, n, stats=st)
        want = retrieval.topn_l2(rt, rows, n)
        assert st['route'] == 'delegate'
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt, score='bf16x3', wide='resident')
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(torch.zeros(30, 32769, device=dev), wide='resident')
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(rt, positions=_traverse(300), wide='resident').query(
            qt[:2], 30, near=_traverse(300)[:2], radius=5.0)             # a window with n > 25
    # at 256 columns or fewer 'resident' is the route there is
    narrow = retrieval.RetrievalIndex(rt[:, :64].contiguous(), wide='resident')
    st = {}
    got = narrow.query(qt[:3, :64].contiguous(), 5, stats=st)
    want = retrieval.RetrievalIndex(rt[:, :64].contiguous()).query(qt[:3, :64].contiguous(), 5)
    assert st['route'] == 'stream' and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 2. integer-valued descriptors: every sum exact, both tensors bit for bit ---------------------------
@pytest.mark.parametrize("r,q,d,n", [(1500, 9, 512, 25), (700, 5, 4096, 5)])
def test_integer_valued_sets_are_bit_exact(dev, r, q, d, n):
    from soft_contrastive_learning_amd.evaluation import retrieval
    rng = np.random.default_rng(d)
    ref = rng.integers(-4, 5, (r, d)).astype(np.float32)
    qry = rng.integers(-4, 5, (q, d)).astype(np.float32)
    ref[r - 1] = ref[40] = ref[7]                                        # exact ties: lower index first
    qry[0] = ref[7]
    qry[1] = ref[100]
    ref[31:34] = ref[100]                                                # ties across a tile boundary
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    st = {}
    got_d, got_i = _index(dev, ref, idx_offset=10 ** 6).query(qt, n, stats=st)
    want_d, want_i = retrieval.topn_l2(rt, qt, n, 10 ** 6)
    assert st['route'] == 'wide' and st['uncertified'] < q, st
    assert torch.equal(got_i, want_i), (got_i, want_i)
    assert torch.equal(got_d, want_d)
    assert got_i[0, :3].tolist() == [10 ** 6 + 7, 10 ** 6 + 40, 10 ** 6 + r - 1] and got_d[0, :3].tolist() == [0.0] * 3
    assert got_i[1, :4].tolist() == [10 ** 6 + k for k in (31, 32, 33, 100)]


# ---- 3. near-duplicate clusters: flagged and resolved ------------------------------------------------------
def test_near_duplicate_clusters(dev):
    """The construction of test_gpu_retrieval_index.test_near_duplicate_clusters at d = 512."""
    from soft_contrastive_learning_amd.evaluation import retrieval
    rng = np.random.default_rng(123)
    r, q, d, n = 6000, 40, 512, 25
    ref = rng.standard_normal((r, d)).astype(np.float32)
    qry = rng.standard_normal((q, d)).astype(np.float32)
    rows_a = rng.permutation(r)[:48]
    ref[rows_a] = qry[3] * (1.0 + 1e-6 * rng.standard_normal((48, 1)).astype(np.float32)) \
        + 1e-6 * rng.standard_normal((48, d)).astype(np.float32)
    rows_b = np.setdiff1d(rng.permutation(r)[:80], rows_a)[:60]
    ref[rows_b] = (qry[7] + 0.01 * rng.standard_normal(d)).astype(np.float32)
    qry = qry[:32]
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    want_d, want_i = TN.topn_kdtree(ref, qry, n)
    l2_d, l2_i = retrieval.topn_l2(rt, qt, n)
    st = {}
    got_d, got_i = _index(dev, ref).query(qt, n, stats=st)
    assert st['route'] == 'wide'
    assert 2 <= st['uncertified'] <= 6, st
    gi = got_i.cpu().numpy()
    np.testing.assert_array_equal(gi[3], want_i[3])
    assert list(gi[7]) == np.sort(rows_b)[:n].tolist()
    ok = np.ones(32, bool)
    ok[7] = False                                   # (the tree may order exact ties differently)
    np.testing.assert_array_equal(gi[ok], want_i[ok])
    assert torch.equal(got_i, l2_i)
    _close(got_d, l2_d, d)
    _close(got_d, want_d, d)


# ---- 4. windows ---------------------------------------------------------------------------------------------
def _assert_window_result(got, stats, want, d, certified=True):
    (got_d, got_i), (want_d, want_i, want_c) = got, want
    assert stats['route'] == 'window'
    np.testing.assert_array_equal(stats['count'].cpu().numpy(), want_c)
    assert stats['count'].dtype == torch.int32
    assert torch.equal(got_i, want_i), (got_i, want_i)
    _close(got_d, want_d, d)                                             # (inf where the window has no more)
    if certified:
        assert stats['uncertified'] == 0, stats


@pytest.mark.parametrize("d,permuted", [(512, False), (512, True), (2048, False)],
                         ids=['512-traverse', '512-permuted', '2048-traverse'])
def test_window_sizes_around_every_threshold(dev, d, permuted):
    """The windows of test_gpu_retrieval_window.test_window_sizes_around_every_threshold — 0, 1, 24,
    25, 26, 31, 32, 33, 200 and R members, the boundary reference exactly on the circle, across tile
    and split boundaries — on a traverse and with positions permuted against the rows."""
    r, q, n = 4099, 32, 25
    ref, qry = U.retrieval_sets(r, q, d)
    xy, near, radius = _threshold_case()
    if permuted:
        xy = xy[np.random.default_rng(4).permutation(r)]
    want = _expected(dev, ref, qry, xy, near, radius, n, kdtree=d == 512 and not permuted)
    assert sorted(set(want[2].tolist())) == [0, 1, 24, 25]
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, want, d)
    gi, gd = got[1].cpu().numpy(), got[0].cpu().numpy()
    for k in range(q):
        c = want[2][k]
        assert (gi[k, c:] == -1).all() and np.isinf(gd[k, c:]).all() and (gi[k, :c] >= 0).all()
        assert set(gi[k, :c]) <= set(_window(xy, near[k], radius[k]))


def test_boundary_radius_zero_negative_and_nan(dev):
    """test_gpu_retrieval_window.test_boundary_is_inclusive_and_exact at d = 512, with an offset."""
    r, d, n = 200, 512, 5
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
    got = _index(dev, ref, xy, 1000).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, _expected(dev, ref, qry, xy, near, radius, n, idx_offset=1000), d)
    gi = got[1].cpu().numpy()
    assert sorted(gi[0]) == sorted(1000 + k for k in on)                 # all five, none of the two beyond
    assert sorted(gi[1]) == [-1, -1, -1, -1, 1033]                       # a radius one ulp short of 5
    assert sorted(gi[2]) == [-1, -1, -1, 1060, 1061]                     # radius 0: the spot itself
    assert (gi[3] == -1).all() and (gi[4] == -1).all()                   # negative, NaN: empty; -1 stays -1
    assert sorted(gi[5]) == [-1, -1, -1, -1, 1033]                       # -0.0 is a radius of zero
    assert st['count'].tolist() == [5, 1, 2, 0, 0, 1]


def test_more_than_32_windowed_queries_go_in_groups(dev):
    r, q, d, n = 3000, 70, 512, 5
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    near, radius = xy[(np.arange(q) * 41) % r], np.linspace(0.0, 30.0, q)
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, _expected(dev, ref, qry, xy, near, radius, n), d)


def test_near_duplicates_inside_a_window_are_resolved_among_its_members(dev):
    rng = np.random.default_rng(77)
    r, q, d, n = 3000, 8, 512, 25
    ref, qry = U.retrieval_sets(r, q, d)
    rows_b = np.sort(rng.permutation(r)[:120])
    ref[rows_b] = (qry[2] + 0.01 * rng.standard_normal(d)).astype(np.float32)   # 120 exact duplicates
    xy = rng.uniform(-50.0, 50.0, (r, 2))
    outside = np.concatenate([rows_b[::2], rng.permutation(r)[:700]])
    xy[outside] += (400.0, 0.0)
    near, radius = np.zeros((q, 2)), 100.0
    want = _expected(dev, ref, qry, xy, near, radius, n)
    st = {}
    got = _index(dev, ref, xy).query(torch.tensor(qry, device=dev), n, stats=st, near=near, radius=radius)
    _assert_window_result(got, st, want, d, certified=False)
    assert 1 <= st['uncertified'] <= 2, st
    gi = got[1].cpu().numpy()
    assert not np.isin(gi, outside).any()
    assert list(gi[2]) == np.setdiff1d(rows_b, outside)[:n].tolist()     # exact ties: ascending row


# ---- 5. every block between guard bands ------------------------------------------------------------------
def _between_bands(dev, fill, windowed, r=8197, q=8, d=512, n=5):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    ref, qry = U.retrieval_sets(r, q, d)
    xy = _traverse(r)
    centres = np.array([0, 31, 32, 1025, 4097, 8196, 8165, 5000])
    near, radius = xy[centres], np.array([3.0, 40.0, 0.0, 100.0, -1.0, 50.0, 1.5, 1e9])
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    xt, ct, rad = (torch.tensor(a, device=dev) for a in (xy, near, radius))
    index = _Guarded(dev, lib.scl_topn_wide_index_bytes(r, d), fill)
    L.check(lib.scl_topn_wide_index_build(L.ptr(rt), r, d, L.ptr(index.inner), index.inner.numel(), L.stream_of(rt)))
    index.assert_bands_intact()
    geo = _Guarded(dev, lib.scl_topn_geo_bytes(r), fill)
    L.check(lib.scl_topn_geo_build(L.ptr(xt), r, L.ptr(geo.inner), geo.inner.numel(), L.stream_of(rt)))
    ws = _Guarded(dev, lib.scl_topn_wide_query_workspace_bytes(r, q, d, n), fill)
    idx, dist, count = _Guarded(dev, q * n * 8, FILL), _Guarded(dev, q * n * 8, FILL), _Guarded(dev, q * 4, FILL)
    flag = torch.ones(q, dtype=torch.uint8, device=dev)
    bound = torch.full((q,), -1.0, dtype=torch.float64, device=dev)
    win = (L.ptr(geo.inner), geo.inner.numel()) if windowed else (None, 0)
    L.check(lib.scl_topn_wide_query(
        L.ptr(rt), r, d, L.ptr(index.inner), index.inner.numel(), *win, L.ptr(qt), q,
        L.ptr(ct) if windowed else None, L.ptr(rad) if windowed else None, n, 0, L.ptr(idx.inner),
        L.ptr(dist.inner), L.ptr(count.inner) if windowed else None, L.ptr(flag), L.ptr(bound),
        L.ptr(ws.inner), ws.inner.numel(), L.stream_of(rt)))
    for g in (index, geo, ws, idx, dist, count):
        g.assert_bands_intact()
    out = [idx.inner.view(torch.int64).view(q, n).clone(), dist.inner.view(torch.float64).view(q, n).clone(),
           flag, bound]
    pat = torch.full((8,), FILL, dtype=torch.uint8, device=dev)          # every output element was written
    assert not bool((out[0] == pat.view(torch.int64)).any())
    assert not bool((out[1] == pat.view(torch.float64)).any())
    assert int(flag.sum()) == 0 and bool((bound >= 0).all())
    if windowed:
        out.append(count.inner.view(torch.int32).clone())
        assert not bool((out[4] == pat[:4].view(torch.int32)).any())
        want_d, want_i, want_c = _expected(dev, ref, qry, xy, near, radius, n)
        np.testing.assert_array_equal(out[4].cpu().numpy(), want_c)
        assert want_c.tolist() == [3, 5, 1, 5, 0, 5, 3, 5]
    else:
        from soft_contrastive_learning_amd.evaluation import retrieval
        want_d, want_i = retrieval.topn_l2(rt, qt, n)
        assert bool((count.inner == FILL).all())                         # not an output of this call
    assert torch.equal(out[0], want_i)
    _close(out[1], want_d, d)
    return out


@pytest.mark.parametrize("windowed", [False, True], ids=['plain', 'window'])
def test_blocks_and_outputs_between_guard_bands(dev, windowed):
    a, b = _between_bands(dev, FILL, windowed), _between_bands(dev, 0, windowed)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                         # nothing is read before it is written


# ---- 6. no state between calls --------------------------------------------------------------------------
def test_no_state_between_calls(dev):
    ref, qry = U.retrieval_sets(5000, 32, 512)
    ref2, _ = U.retrieval_sets(3000, 1, 1280, seed_r=21)
    qry2 = U.retrieval_sets(1, 32, 1280)[1]
    xy = _traverse(5000)
    qt, qt2 = torch.tensor(qry, device=dev), torch.tensor(qry2, device=dev)
    win = (xy[np.arange(32) * 150], np.full(32, 60.0))
    one, other = _index(dev, ref, xy), _index(dev, ref2)
    first = one.query(qt, 25)
    o1 = other.query(qt2, 7)
    windowed = one.query(qt, 25, near=win[0], radius=win[1])
    o2 = other.query(qt2[:3], 7)
    few = one.query(qt[:1], 25)
    last = one.query(qt, 25)
    o3 = other.query(qt2, 7)
    assert torch.equal(first[0], last[0]) and torch.equal(first[1], last[1])
    assert torch.equal(o1[0], o3[0]) and torch.equal(o1[1], o3[1])
    assert torch.equal(o2[0], o1[0][:3]) and torch.equal(o2[1], o1[1][:3])
    assert torch.equal(few[0], first[0][:1]) and torch.equal(few[1], first[1][:1])
    fresh = _index(dev, ref, xy).query(qt, 25, near=win[0], radius=win[1])
    assert torch.equal(windowed[0], fresh[0]) and torch.equal(windowed[1], fresh[1])
    assert not torch.equal(windowed[1], first[1])


# ---- 7. the localiser and the command, at 512 whitened columns ------------------------------------------
def _course(m, e=2048, seed=5):
    """A traverse of m references 1 m apart, descriptors [m, e], frames (noisy copies of every third
    reference) with their positions, and 640 more rows to fit a PCA on."""
    rng = np.random.default_rng(seed)
    x = np.arange(m, dtype=np.float64)
    ref_xy = np.stack([620000.25 + x, 5735000.5 + 0.5 * np.sin(x / 50.0)], 1)
    ref_f = rng.standard_normal((m, e)).astype(np.float32)
    rows = np.arange(2, m, 3)
    qry_f = (ref_f[rows] + 0.05 * rng.standard_normal((len(rows), e))).astype(np.float32)
    pca_f = rng.standard_normal((640, e)).astype(np.float32)            # the PCA is fitted on rows of its own
    return ref_xy, ref_f, rows, qry_f, ref_xy[rows] + 0.25, pca_f


def test_localizer_resident_against_delegate(dev):
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.evaluation.pca import PCAWhitening
    n, d = 5, 512
    ref_xy, ref_f, rows, qry_f, qry_xy, pca_f = _course(640)
    pca = PCAWhitening(d, device='cuda').fit(pca_f)
    res = localize.Localizer(ref_f, ref_xy, pca=pca, n=n, device=dev, wide='resident')
    dele = localize.Localizer(ref_f, ref_xy, pca=pca, n=n, device=dev)
    assert res._index.width == d and res._index._wide and not dele._index._wide
    qry_f = qry_f[:40]
    idx, fd, xy = res.locate_descriptors(qry_f)
    idx0, fd0, xy0 = dele.locate_descriptors(qry_f)
    np.testing.assert_array_equal(idx, idx0)
    np.testing.assert_allclose(fd, fd0, rtol=_rtol(d), atol=0)
    np.testing.assert_array_equal(xy, xy0)
    assert list(idx[:, 0]) == list(rows[:40]) and res.uncertified == 0
    # with a window: the delegate refuses, the resident index answers what the subset gives
    radius = np.linspace(0.0, 12.0, 40)
    radius[5], radius[6] = -1.0, 1e9
    with pytest.raises(ValueError):
        dele.locate_descriptors(qry_f, near=qry_xy[:40], radius=radius)
    idx, fd, xy = res.locate_descriptors(qry_f, near=qry_xy[:40], radius=radius)
    white_r = res._index.ref[:, :d].cpu().numpy()
    white_q = res._whiten(qry_f).cpu().numpy()
    kept = np.asarray(res.ref_idx)                                       # the index's rows -> original indices
    want_d, want_i, want_c = _expected(dev, white_r, white_q, ref_xy[kept], qry_xy[:40], radius, n)
    want_i = want_i.cpu().numpy()
    assert 0 in want_c and n in want_c and ((want_c > 0) & (want_c < n)).any()
    np.testing.assert_array_equal(idx, np.where(want_i >= 0, kept[np.maximum(want_i, 0)], -1))
    np.testing.assert_allclose(fd, want_d.cpu().numpy(), rtol=_rtol(d), atol=0)
    np.testing.assert_array_equal(xy, np.where((idx >= 0)[..., None], ref_xy[np.maximum(idx, 0)], np.nan))
    assert res.uncertified == 0


def test_command_with_the_wide_index(dev, tmp_path, capsys):
    """``evaluation.localize --D 512 --wide_index 1`` against the same command without the flag, the
    PCA fitted on 640 rows of 2048; then with a prior, which the command without the flag refuses."""
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.util import io
    n, d, batch, radius = 5, 512, 2, 12.0
    ref_xy, ref_f, rows, qry_f, qry_xy, pca_f = _course(640)
    rows, qry_f, qry_xy = rows[:60], qry_f[:60], qry_xy[:60]
    for name, f in (('ref', ref_f), ('query', qry_f), ('pca', pca_f)):
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
                              '--N', str(n), '--out_root', str(tmp_path / out), '--L', '0', '--D', str(d),
                              '--score', 'f32', '--batch', str(batch), *more])
        return io.load_pickle(path), capsys.readouterr().out
    plain, said0 = run('plain')
    wide, said1 = run('wide', '--wide_index', '1')
    assert 'uncertified 0' in said0 and 'uncertified 0' in said1
    np.testing.assert_array_equal(np.asarray(wide[0]), np.asarray(plain[0]))          # the index lists
    np.testing.assert_allclose(np.asarray(wide[2]), np.asarray(plain[2]), rtol=_rtol(d), atol=0)
    np.testing.assert_array_equal(np.asarray(wide[1]), np.asarray(plain[1]))          # geographic: same hits
    assert list(np.asarray(wide[0])[:, 0]) == list(rows)                 # it tracks
    with pytest.raises(ValueError):
        run('plain_prior', '--prior_radius', str(radius))                # no window without the wide index
    with pytest.raises(ValueError):
        run('bf', '--wide_index', '1', '--score', 'bf16x3')              # the wide index scores in float32
    prior, said = run('prior', '--wide_index', '1', '--prior_radius', str(radius))
    top_i, free = np.asarray(prior[0]), np.asarray(wide[0])
    assert list(top_i[:, 0]) == list(rows)
    again = 0
    for s in range(batch, len(rows), batch):
        inside = _window(ref_xy, ref_xy[top_i[s - 1, 0]], radius)
        for k in range(s, min(s + batch, len(rows))):
            if len(inside) < n:                                          # searched again, everywhere
                again += 1
                np.testing.assert_array_equal(top_i[k], free[k])
            else:                                                        # every hit within the window
                assert np.isin(top_i[k], inside).all(), k
    assert int(re.search(r'(\d+) frames searched again', said).group(1)) == again
    assert (top_i != free).any()                                         # the prior did restrict something

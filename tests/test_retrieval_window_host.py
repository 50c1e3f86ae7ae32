"""Host-side checks of retrieval with a position prior (no GPU): the C-ABI additions of
include/scl_hip.h (declared, bound, size queries, every refusal before any launch) and the
bookkeeping of evaluation/localize.py around a NumPy stand-in for the index."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")
NEW = ("scl_topn_geo_bytes", "scl_topn_geo_build", "scl_topn_index_query_window_workspace_bytes",
       "scl_topn_index_query_window")
F32, BF = 0, 1
E_SHAPE, E_KIND, E_NULL, E_WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_header_declares_and_lib_binds_the_window_calls():
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["scl_topn_index_query_window"][1]) == 22
    assert re.search(r"#define\s+SCL_ABI_VERSION\s+12\b", src)          # purely additive
    assert _lib.ABI_VERSION == 12


def _r256(nbytes):
    return (nbytes + 255) // 256 * 256


def _stream_splits(r):
    """stream_plan of csrc/topn.hip: at most 32 lists, each over at least one selection step"""
    s = min(-(-r // 1024), 32)
    per = -(-r // s)
    return -(-r // per)


def test_sizes_are_those_of_the_hand_carved_layouts(lib):
    for r in (25, 1000, 4099, 100003):
        # xy [R][2] float64 | one box of 4 float64 per 32-reference tile, each piece rounded to 256
        assert lib.scl_topn_geo_bytes(r) == _r256(16 * r) + _r256(32 * -(-r // 32)), r
        for d in (32, 256):
            for q in (1, 8, 32):
                for flags in (F32, BF):
                    n = min(25, r)
                    lists = _r256(4 * q * _stream_splits(r) * 32)
                    want = _r256(4 * q * r) + 2 * lists          # scores [Q][R] | cs | ci [Q][splits][32]
                    got = lib.scl_topn_index_query_window_workspace_bytes(r, q, d, n, flags)
                    assert got == want, (r, q, d, flags)
                    # the stream route's own workspace: one layout
                    assert got == lib.scl_topn_index_query_workspace_bytes(r, q, d, n, flags)
    assert lib.scl_topn_geo_bytes(0) == 0 and lib.scl_topn_geo_bytes(-5) == 0
    ws = lib.scl_topn_index_query_window_workspace_bytes
    assert ws(1000, 33, 64, 5, F32) == 0                                 # more than the stream route takes
    assert ws(1000, 0, 64, 5, F32) == 0 and ws(0, 4, 64, 5, F32) == 0
    assert ws(1000, 4, 100, 5, F32) == 0 and ws(1000, 4, 64, 26, F32) == 0
    assert ws(10, 4, 64, 11, F32) == 0 and ws(1000, 4, 64, 5, 2) == 0


def _p(v):
    return ctypes.c_void_p(v)


def test_every_refusal_comes_before_any_launch(lib):
    """This test runs without a GPU; the pointers are aligned numbers, never dereferenced."""
    r, d, q, n = 1000, 64, 4, 5
    a = 1 << 20                                                          # 256-byte aligned
    gb = lib.scl_topn_geo_bytes(r)
    ib = lib.scl_topn_index_bytes(r, d, F32)
    wb = lib.scl_topn_index_query_window_workspace_bytes(r, q, d, n, F32)

    def build(xy=a, rr=r, geo=2 * a, nbytes=gb):
        return lib.scl_topn_geo_build(_p(xy), rr, _p(geo), nbytes, None)

    assert build(xy=None) == E_NULL and build(geo=None) == E_NULL
    assert build(rr=0) == E_SHAPE and build(xy=a + 4) == E_SHAPE
    assert build(nbytes=gb - 1) == E_WORKSPACE and build(geo=2 * a + 16) == E_WORKSPACE
    assert build(xy=None, rr=0, nbytes=0) == E_NULL                      # order: NULL first
    assert build(rr=0, nbytes=0) == E_SHAPE                              # then shape, then the block

    def query(ref=a, index=2 * a, ibytes=ib, geo=3 * a, gbytes=gb, qry=4 * a, qq=q, center=5 * a,
              radius=6 * a, nn=n, dd=d, idx=7 * a, dist=8 * a, count=9 * a, unc=10 * a, bound=11 * a,
              ws=12 * a, wbytes=wb, flags=F32):
        return lib.scl_topn_index_query_window(_p(ref), r, dd, _p(index), ibytes, _p(geo), gbytes, _p(qry),
                                               qq, _p(center), _p(radius), nn, 0, _p(idx), _p(dist),
                                               _p(count), _p(unc), _p(bound), _p(ws), wbytes, flags, None)

    for name in ('ref', 'index', 'geo', 'qry', 'center', 'radius', 'idx', 'dist', 'count', 'ws'):
        assert query(**{name: None}) == E_NULL, name
    assert query(unc=None) == E_NULL and query(bound=None) == E_NULL     # both or neither
    assert query(qq=33) == E_SHAPE                                       # the stream route only
    assert query(dd=100) == E_SHAPE and query(nn=26) == E_SHAPE and query(nn=r + 1) == E_SHAPE
    assert query(qq=0) == E_SHAPE
    assert query(ref=a + 4) == E_SHAPE and query(qry=4 * a + 8) == E_SHAPE
    assert query(center=5 * a + 4) == E_SHAPE and query(radius=6 * a + 4) == E_SHAPE
    assert query(ibytes=ib - 1) == E_WORKSPACE and query(index=2 * a + 128) == E_WORKSPACE
    assert query(gbytes=gb - 1) == E_WORKSPACE and query(geo=3 * a + 128) == E_WORKSPACE
    assert query(wbytes=wb - 1) == E_WORKSPACE and query(ws=12 * a + 64) == E_WORKSPACE
    assert query(flags=2) == E_KIND
    assert query(flags=BF) == E_WORKSPACE                                # the index block lacks the planes
    # order of precedence: NULL, shape / alignment, workspace, flags
    assert query(unc=None, qq=33, wbytes=0, flags=2) == E_NULL
    assert query(qq=33, wbytes=0, flags=2) == E_SHAPE
    assert query(center=5 * a + 4, gbytes=0, flags=2) == E_SHAPE
    assert query(gbytes=0, flags=2) == E_WORKSPACE
    assert query(wbytes=0, flags=2) == E_WORKSPACE


# ---- Localizer bookkeeping around a NumPy stand-in for the index -------------------------------------
def _numpy_topn(ref_f, query_f, n):
    r64, q64 = np.asarray(ref_f, np.float64), np.asarray(query_f, np.float64)
    d2 = ((q64[:, None, :] - r64[None]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :n]
    return np.sqrt(np.take_along_axis(d2, idx, 1)), idx


def _track(m=120, q=23, e=24, seed=5):
    """References along a track 0.5 m apart (thinning at 1.2 m drops most of them), queries near it."""
    rng = np.random.default_rng(seed)
    ref_xy = np.stack([620000.25 + 0.5 * np.arange(m), 5735000.5 + 0.1 * rng.standard_normal(m)], 1)
    qry_xy = np.stack([620000.25 + rng.uniform(0, 0.5 * m, q), 5735000.5 + rng.standard_normal(q)], 1)
    ref_f = rng.standard_normal((m, e)).astype(np.float32)
    qry_f = rng.standard_normal((q, e)).astype(np.float32)
    return ref_xy, qry_xy, ref_f, qry_f


def _restated(ref_f, ref_xy, kept, qry_f, near, radius, n):
    """The semantics, literally: per query the window over the kept references, the exact top
    min(n, |W|) of those rows by (distance, index), original indices, then (-1, inf, NaN)."""
    q = len(qry_f)
    idx = np.full((q, n), -1, dtype=np.int64)
    dist = np.full((q, n), np.inf)
    xy = np.full((q, n, 2), np.nan)
    kept = np.asarray(kept)
    for k in range(q):
        dx = ref_xy[kept, 0] - near[k, 0]
        dy = ref_xy[kept, 1] - near[k, 1]
        w = kept[(radius[k] >= 0) & (dx * dx + dy * dy <= radius[k] * radius[k])]
        d2 = ((qry_f[k].astype(np.float64) - ref_f[w].astype(np.float64)) ** 2).sum(-1)
        o = np.argsort(d2, kind='stable')[:n]
        idx[k, :len(o)], dist[k, :len(o)], xy[k, :len(o)] = w[o], np.sqrt(d2[o]), ref_xy[w[o]]
    return idx, dist, xy


@pytest.mark.parametrize("l", [0.0, 1.2])
def test_localizer_window_matches_the_restated_semantics(l):
    from soft_contrastive_learning_amd.evaluation import localize
    ref_xy, qry_xy, ref_f, qry_f = _track()
    loc = localize.Localizer(ref_f, ref_xy, n=5, l=l, query_fn=_numpy_topn)
    q = len(qry_f)
    radius = np.linspace(0.0, 8.0, q)
    radius[3], radius[4], radius[5] = -1.0, np.nan, 1e9
    idx, fd, xy = loc.locate_descriptors(qry_f, near=qry_xy, radius=radius)
    want_i, want_d, want_xy = _restated(ref_f, ref_xy, loc.ref_idx, qry_f, qry_xy, radius, 5)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_allclose(fd, want_d, rtol=1e-12)
    np.testing.assert_array_equal(xy, want_xy)
    assert (idx[3] == -1).all() and (idx[4] == -1).all() and np.isinf(fd[3]).all() and np.isnan(xy[4]).all()
    counts = (idx >= 0).sum(1)
    assert 0 in counts and 5 in counts and ((counts > 0) & (counts < 5)).any()    # every kind of row
    # a scalar radius and one centre for all frames
    idx1, fd1, _ = loc.locate_descriptors(qry_f, near=qry_xy[7], radius=4.0)
    want_i, want_d, _ = _restated(ref_f, ref_xy, loc.ref_idx, qry_f, np.tile(qry_xy[7], (q, 1)),
                                  np.full(q, 4.0), 5)
    np.testing.assert_array_equal(idx1, want_i)
    np.testing.assert_allclose(fd1, want_d, rtol=1e-12)
    # a window that holds everything is no window; neither is none
    idx2, fd2, xy2 = loc.locate_descriptors(qry_f, near=qry_xy, radius=1e9)
    idx3, fd3, xy3 = loc.locate_descriptors(qry_f)
    np.testing.assert_array_equal(idx2, idx3)
    np.testing.assert_array_equal(fd2, fd3)
    np.testing.assert_array_equal(xy2, xy3)
    with pytest.raises(ValueError):
        loc.locate_descriptors(qry_f, near=qry_xy)                       # half a window


def _write_set(tmp_path, ref_xy, qry_xy, ref_f, qry_f):
    from soft_contrastive_learning_amd.util import io
    for name, f in (('ref', ref_f), ('query', qry_f), ('pca', ref_f)):
        io.save_pickle([row for row in f], str(tmp_path / ('set_%s.v1.pickle' % name)))
    for name, xy in (('ref', ref_xy), ('query', qry_xy)):
        io.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]],
                     'northing': [repr(float(v)) for v in xy[:, 1]]}, str(tmp_path / ('%s.csv' % name)))

    def argv(out_root, *more):
        return ['--pca_lv_pickle', str(tmp_path / 'set_pca.v1.pickle'),
                '--query_lv_pickle', str(tmp_path / 'set_query.v1.pickle'),
                '--ref_lv_pickle', str(tmp_path / 'set_ref.v1.pickle'),
                '--query_csv', str(tmp_path / 'query.csv'), '--ref_csv', str(tmp_path / 'ref.csv'),
                '--N', '5', '--out_root', str(tmp_path / out_root), '--L', '0', '--D', '0', *more]
    return argv


def test_command_prior_radius_on_and_off(tmp_path, capsys):
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.util import io
    ref_xy, qry_xy, ref_f, qry_f = _track()
    argv = _write_set(tmp_path, ref_xy, qry_xy, ref_f, qry_f)
    off = localize.main(argv('off', '--batch', '3'), query_fn=_numpy_topn)
    assert 'searched again' not in capsys.readouterr().out
    zero = localize.main(argv('zero', '--batch', '3', '--prior_radius', '0'), query_fn=_numpy_topn)
    assert open(off, 'rb').read() == open(zero, 'rb').read()             # 0 = off, byte for byte
    capsys.readouterr()
    huge = localize.main(argv('huge', '--batch', '3', '--prior_radius', '1e9'), query_fn=_numpy_topn)
    assert 'prior radius 1e+09 m: 0 frames searched again' in capsys.readouterr().out
    assert open(off, 'rb').read() == open(huge, 'rb').read()             # a window that holds everything

    radius, batch, n = 1.01, 3, 5        # holds the 5 references within 1 m along the track, or fewer
    out = localize.main(argv('on', '--batch', str(batch), '--prior_radius', str(radius)), query_fn=_numpy_topn)
    said = capsys.readouterr().out
    top_i = np.asarray(io.load_pickle(out)[0])
    free = np.asarray(io.load_pickle(off)[0])
    assert top_i.shape == free.shape == (len(qry_f), n)
    again = 0
    for s in range(0, len(qry_f), batch):
        rows = range(s, min(s + batch, len(qry_f)))
        if s == 0:                                                       # no prior yet
            np.testing.assert_array_equal(top_i[:batch], free[:batch])
            continue
        prior = ref_xy[top_i[s - 1, 0]]
        dx, dy = ref_xy[:, 0] - prior[0], ref_xy[:, 1] - prior[1]
        inside = dx * dx + dy * dy <= radius * radius
        for k in rows:
            if inside.sum() < n:                                         # searched again, everywhere
                again += 1
                np.testing.assert_array_equal(top_i[k], free[k])
            else:
                assert inside[top_i[k]].all(), k
                d2 = ((qry_f[k].astype(np.float64) - ref_f[inside].astype(np.float64)) ** 2).sum(-1)
                np.testing.assert_array_equal(top_i[k], np.nonzero(inside)[0][np.argsort(d2, kind='stable')[:n]])
    assert 'prior radius 1.01 m: %d frames searched again' % again in said
    assert 0 < again < len(qry_f) - batch                                # both kinds of frame occurred
    assert (top_i != free).any()                                         # the prior did restrict something

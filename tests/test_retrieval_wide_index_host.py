"""Host-side checks of the resident index for descriptors wider than 256 columns (no GPU): the C-ABI
additions of include/scl_hip.h (declared, bound, size queries, every refusal of
``scl_topn_wide_query`` before any launch) and the Python arguments in front of them."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")
NEW = ("scl_topn_wide_index_bytes", "scl_topn_wide_index_build", "scl_topn_wide_query_workspace_bytes",
       "scl_topn_wide_query")
E_SHAPE, E_NULL, E_WORKSPACE = -1, -3, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_header_declares_and_lib_binds_the_wide_calls():
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    # the arguments of scl_topn_index_query_window minus flags
    window = _lib.SIGNATURES["scl_topn_index_query_window"][1]
    assert _lib.SIGNATURES["scl_topn_wide_query"][1] == window[:20] + window[21:]
    assert re.search(r"#define\s+SCL_ABI_VERSION\s+12\b", src)          # purely additive
    assert _lib.ABI_VERSION == 12


def _r256(nbytes):
    return (nbytes + 255) // 256 * 256


def _stream_splits(r):
    """stream_plan of csrc/topn.hip: at most 32 lists, each over at least one selection step"""
    s = min(-(-r // 1024), 32)
    per = -(-r // s)
    return -(-r // per)


def test_sizes_are_non_zero_and_aligned_where_supported(lib):
    for r in (25, 1000, 4099, 100003):
        for d in (512, 768, 1024, 4096, 32768):
            ib = lib.scl_topn_wide_index_bytes(r, d)
            assert ib == 256 + _r256(4 * r), (r, d)                      # the bound word | refnorm [R]
            for q in (1, 8, 32):
                for n in (1, min(25, r)):
                    got = lib.scl_topn_wide_query_workspace_bytes(r, q, d, n)
                    assert got > 0 and got % 256 == 0
                    # scores [Q][R] | cs | ci [Q][splits][32]: the stream route's one layout
                    assert got == _r256(4 * q * r) + 2 * _r256(4 * q * _stream_splits(r) * 32), (r, q, d, n)
                    assert got == lib.scl_topn_index_query_workspace_bytes(r, q, 256, n, 0)


def test_sizes_are_zero_for_what_the_route_does_not_take(lib):
    ws, ib = lib.scl_topn_wide_query_workspace_bytes, lib.scl_topn_wide_index_bytes
    assert ws(1000, 4, 512, 5) > 0 and ib(1000, 512) > 0
    for d in (256, 300, 33024, 0, -512, 520):
        assert ws(1000, 4, d, 5) == 0, d
        assert ib(1000, d) == 0, d
    assert ws(0, 4, 512, 5) == 0 and ib(0, 512) == 0 and ib(-3, 512) == 0
    assert ws(1000, 33, 512, 5) == 0 and ws(1000, 0, 512, 5) == 0
    assert ws(1000, 4, 512, 26) == 0 and ws(1000, 4, 512, 0) == 0
    assert ws(10, 4, 512, 11) == 0                                       # n > R
    # the entry points for d <= 256 still refuse these widths (topn_shape_ok is unchanged)
    assert lib.scl_topn_index_bytes(1000, 512, 0) == 0
    assert lib.scl_topn_index_query_workspace_bytes(1000, 4, 512, 5, 0) == 0


def _p(v):
    return ctypes.c_void_p(v)


def test_every_refusal_comes_before_any_launch(lib):
    """This test runs without a GPU; the pointers are aligned numbers, never dereferenced."""
    r, d, q, n = 1000, 512, 4, 5
    a = 1 << 20                                                          # 256-byte aligned
    gb = lib.scl_topn_geo_bytes(r)
    ib = lib.scl_topn_wide_index_bytes(r, d)
    wb = lib.scl_topn_wide_query_workspace_bytes(r, q, d, n)

    def build(ref=a, rr=r, dd=d, index=2 * a, nbytes=ib):
        return lib.scl_topn_wide_index_build(_p(ref), rr, dd, _p(index), nbytes, None)

    assert build(ref=None) == E_NULL and build(index=None) == E_NULL
    assert build(rr=0) == E_SHAPE and build(dd=256) == E_SHAPE and build(dd=520) == E_SHAPE
    assert build(dd=33024) == E_SHAPE and build(ref=a + 4) == E_SHAPE
    assert build(nbytes=ib - 1) == E_WORKSPACE and build(index=2 * a + 16) == E_WORKSPACE
    assert build(ref=None, rr=0, nbytes=0) == E_NULL                     # order: NULL first
    assert build(rr=0, nbytes=0) == E_SHAPE                              # then shape, then the block

    def query(ref=a, index=2 * a, ibytes=ib, geo=3 * a, gbytes=gb, qry=4 * a, qq=q, center=5 * a,
              radius=6 * a, nn=n, dd=d, idx=7 * a, dist=8 * a, count=9 * a, unc=10 * a, bound=11 * a,
              ws=12 * a, wbytes=wb):
        return lib.scl_topn_wide_query(_p(ref), r, dd, _p(index), ibytes, _p(geo), gbytes, _p(qry), qq,
                                       _p(center), _p(radius), nn, 0, _p(idx), _p(dist), _p(count), _p(unc),
                                       _p(bound), _p(ws), wbytes, None)

    nowin = dict(geo=None, gbytes=0, center=None, radius=None, count=None)
    for kw in ({}, nowin):                                               # with a window and without
        for name in ('ref', 'index', 'qry', 'idx', 'dist', 'ws'):
            assert query(**{**kw, name: None}) == E_NULL, name
        assert query(**kw, unc=None) == E_NULL and query(**kw, bound=None) == E_NULL   # both or neither
        assert query(**kw, qq=33) == E_SHAPE and query(**kw, qq=0) == E_SHAPE
        assert query(**kw, dd=256) == E_SHAPE and query(**kw, dd=300) == E_SHAPE
        assert query(**kw, dd=33024) == E_SHAPE
        assert query(**kw, nn=26) == E_SHAPE and query(**kw, nn=r + 1) == E_SHAPE and query(**kw, nn=0) == E_SHAPE
        assert query(**kw, ref=a + 4) == E_SHAPE and query(**kw, qry=4 * a + 8) == E_SHAPE
        assert query(**kw, ibytes=ib - 1) == E_WORKSPACE and query(**kw, index=2 * a + 128) == E_WORKSPACE
        assert query(**kw, wbytes=wb - 1) == E_WORKSPACE and query(**kw, ws=12 * a + 64) == E_WORKSPACE
        # order of precedence: NULL, shape / alignment, workspace
        assert query(**kw, unc=None, qq=33, wbytes=0) == E_NULL
        assert query(**kw, qq=33, wbytes=0) == E_SHAPE
        assert query(**kw, ref=a + 4, ibytes=0) == E_SHAPE
    # the window's four arguments come together or not at all
    for name in ('geo', 'center', 'radius', 'count'):
        assert query(**{name: None}) == E_NULL, name
        assert query(**{**nowin, name: 13 * a}) == E_NULL, name
    assert query(geo=None, qq=33, wbytes=0) == E_NULL
    assert query(center=5 * a + 4) == E_SHAPE and query(radius=6 * a + 4) == E_SHAPE
    assert query(gbytes=gb - 1) == E_WORKSPACE and query(geo=3 * a + 128) == E_WORKSPACE
    assert query(center=5 * a + 4, gbytes=0) == E_SHAPE
    assert query(gbytes=0, wbytes=0) == E_WORKSPACE


def test_python_arguments():
    """``wide`` is the last argument everywhere, 'delegate' by default, and is checked before any
    device work (a CPU tensor is refused after it)."""
    import torch

    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.evaluation import localize, retrieval
    sig = inspect.signature(retrieval.RetrievalIndex.__init__)
    assert list(sig.parameters)[1:] == ['ref', 'idx_offset', 'score', 'positions', 'wide']
    assert sig.parameters['wide'].default == 'delegate'
    assert inspect.signature(localize.Localizer.__init__).parameters['wide'].default == 'delegate'
    assert localize.main_parser().parse_args(
        ['--pca_lv_pickle', 'p', '--query_lv_pickle', 'q', '--ref_lv_pickle', 'r', '--query_csv', 'q.csv',
         '--ref_csv', 'r.csv']).wide_index == 0
    assert retrieval.WIDE_MAX == 32768
    with pytest.raises(ValueError):
        retrieval.RetrievalIndex(torch.zeros(10, 512), wide='yes')
    with pytest.raises(_lib.SclError):
        retrieval.RetrievalIndex(torch.zeros(10, 512), wide='resident')   # no CPU fallback

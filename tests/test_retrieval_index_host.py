"""Host-side checks of the prepared retrieval index (no GPU): the C-ABI additions of
include/scl_hip.h (declared, bound, size queries, validation before any launch) and the
bookkeeping of evaluation/localize.py around a NumPy stand-in for the index."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")
NEW = ("scl_topn_index_bytes", "scl_topn_index_build", "scl_topn_index_query_workspace_bytes",
       "scl_topn_index_query")
F32, BF = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_header_declares_and_lib_binds_the_index_calls():
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+SCL_TOPN_STREAM_MAX_Q\s+32\b", src)
    assert _lib.TOPN_STREAM_MAX_Q == 32
    assert re.search(r"#define\s+SCL_ABI_VERSION\s+12\b", src)          # purely additive


def test_size_queries(lib):
    for flags in (F32, BF):
        for r, d in ((25, 32), (1000, 64), (4099, 128), (100003, 256)):
            nb = lib.scl_topn_index_bytes(r, d, flags)
            assert nb > 0 and nb % 256 == 0, (r, d, flags, nb)
            assert nb >= 256 + 4 * r
            for q in (1, 8, 32, 33, 128):
                ws = lib.scl_topn_index_query_workspace_bytes(r, q, d, min(25, r), flags)
                assert ws > 0 and ws % 256 == 0, (r, q, d, flags, ws)
                if q <= 32:
                    assert ws >= 4 * q * r                                # the score matrix
    for r, d in ((1000, 64), (100003, 256)):
        assert lib.scl_topn_index_bytes(r, d, BF) - lib.scl_topn_index_bytes(r, d, F32) >= 2 * r * d * 2
    # unsupported: width, n > 25, n > R, unknown flag
    assert lib.scl_topn_index_bytes(1000, 100, F32) == 0
    assert lib.scl_topn_index_bytes(0, 64, F32) == 0
    assert lib.scl_topn_index_bytes(1000, 64, 2) == 0
    assert lib.scl_topn_index_query_workspace_bytes(1000, 4, 100, 5, F32) == 0
    assert lib.scl_topn_index_query_workspace_bytes(1000, 4, 64, 26, F32) == 0
    assert lib.scl_topn_index_query_workspace_bytes(10, 4, 64, 11, F32) == 0
    assert lib.scl_topn_index_query_workspace_bytes(1000, 4, 64, 5, 4) == 0
    # the scan route's workspace is the one-shot call's without the norms and the planes
    r, q, d, n = 40000, 64, 128, 25
    for flags in (F32, BF):
        planes = lib.scl_topn_index_bytes(r, d, flags) - lib.scl_topn_index_bytes(r, d, F32)
        assert (lib.scl_topn_index_query_workspace_bytes(r, q, d, n, flags)
                == lib.scl_topn_l2_ex_workspace_bytes(r, q, d, n, flags) - planes
                - lib.scl_topn_index_bytes(r, d, F32))


# What the size queries returned BEFORE the layouts were folded into one description each (evaluated on
# that commit's build): the fold may not move a byte.  The NetVLAD rows are for 256 CUs — the count
# the library assumes without a device, and the MI355X's.
_SIZE_QS = (1, 32, 33, 130)
# (R, d, flags): (index_bytes, then per Q of _SIZE_QS: (l2_ex_workspace_bytes, index_query_workspace_bytes))
_TOPN_SIZES = {
    (25, 32, 0): (512, (1024, 768), (8704, 11520), (9216, 8704), (33792, 33280)),
    (25, 32, 1): (4096, (4608, 768), (12288, 11520), (12800, 8704), (37376, 33280)),
    (25, 256, 0): (512, (1024, 768), (8704, 11520), (9216, 8704), (33792, 33280)),
    (25, 256, 1): (26112, (26624, 768), (34304, 11520), (34816, 8704), (59392, 33280)),
    (1000, 32, 0): (4352, (4864, 4608), (12544, 136192), (13056, 8704), (37632, 33280)),
    (1000, 32, 1): (132352, (132864, 4608), (140544, 136192), (141056, 8704), (165632, 33280)),
    (1000, 256, 0): (4352, (4864, 4608), (12544, 136192), (13056, 8704), (37632, 33280)),
    (1000, 256, 1): (1028352, (1028864, 4608), (1036544, 136192), (1037056, 8704), (1061632, 33280)),
    (32767, 32, 0): (131328, (139520, 139264), (393472, 4456448), (401664, 270336), (1196288, 1064960)),
    (32767, 32, 1): (4325632, (4333824, 139264), (4587776, 4456448), (4595968, 270336), (5390592, 1064960)),
    (32767, 256, 0): (131328, (139520, 139264), (393472, 4456448), (401664, 270336), (1196288, 1064960)),
    (32767, 256, 1): (33684736, (33692928, 139264), (33946880, 4456448), (33955072, 270336), (34749696, 1064960)),
    (32768, 32, 0): (131328, (166656, 139264), (1249792, 4456448), (1284864, 1153536), (4674816, 4543488)),
    (32768, 32, 1): (4325632, (4360960, 139264), (5444096, 4456448), (5479168, 1153536), (8869120, 4543488)),
    (32768, 256, 0): (131328, (166656, 139264), (1249792, 4456448), (1284864, 1153536), (4674816, 4543488)),
    (32768, 256, 1): (33685760, (33721088, 139264), (34804224, 4456448), (34839296, 1153536), (38229248, 4543488)),
    (100003, 32, 0): (400384, (435712, 408320), (1518848, 13062656), (1553920, 1153536), (4943872, 4543488)),
    (100003, 32, 1): (13200896, (13236224, 408320), (14319360, 13062656), (14354432, 1153536), (17744384, 4543488)),
    (100003, 256, 0): (400384, (435712, 408320), (1518848, 13062656), (1553920, 1153536), (4943872, 4543488)),
    (100003, 256, 1): (102803456, (102838784, 408320), (103921920, 13062656), (103956992, 1153536),
                       (107346944, 4543488)),
}
_NETVLAD_SIZES = {    # (B, N): (fwd_workspace_bytes, bwd_workspace_bytes)
    (1, 1): (1061120, 2370304),
    (2, 37): (1746176, 3447296),
    (24, 1200): (42818560, 53104128),
    (144, 300): (107555584, 164902656),
}


def test_sizes_are_those_of_the_hand_carved_layouts(lib):
    for (r, d, flags), (index_bytes, *per_q) in _TOPN_SIZES.items():
        assert lib.scl_topn_index_bytes(r, d, flags) == index_bytes, (r, d, flags)
        for q, (l2_ws, query_ws) in zip(_SIZE_QS, per_q):
            n = min(25, r)
            assert lib.scl_topn_l2_ex_workspace_bytes(r, q, d, n, flags) == l2_ws, (r, q, d, flags)
            assert lib.scl_topn_index_query_workspace_bytes(r, q, d, n, flags) == query_ws, (r, q, d, flags)
    for (b, n), (fwd, bwd) in _NETVLAD_SIZES.items():
        assert lib.scl_netvlad_fwd_workspace_bytes(b, n) == fwd, (b, n)
        assert lib.scl_netvlad_bwd_workspace_bytes(b, n) == bwd, (b, n)


def test_one_shot_workspace_is_index_block_plus_scan_lists(lib):
    """scl_topn_l2_cert's workspace = index block | candidate lists, and the scan route of
    scl_topn_index_query needs exactly those lists."""
    for r, d, flags in _TOPN_SIZES:
        for q in (33, 130):
            n = min(25, r)
            assert (lib.scl_topn_index_query_workspace_bytes(r, q, d, n, flags)
                    == lib.scl_topn_l2_ex_workspace_bytes(r, q, d, n, flags)
                    - lib.scl_topn_index_bytes(r, d, flags)), (r, q, d, flags)


def _p(v):
    return ctypes.c_void_p(v)


def test_validation_before_any_launch(lib):
    """Every rejection below returns before the first HIP call (this test runs without a GPU; the
    pointers are aligned numbers, never dereferenced)."""
    r, d, q, n = 1000, 64, 4, 5
    a = 1 << 20                                                          # 256-byte aligned
    ib = lib.scl_topn_index_bytes(r, d, F32)
    wb = lib.scl_topn_index_query_workspace_bytes(r, q, d, n, F32)

    def build(ref=a, rr=r, dd=d, index=2 * a, nbytes=ib, flags=F32):
        return lib.scl_topn_index_build(_p(ref), rr, dd, _p(index), nbytes, flags, None)

    assert build(ref=None) == -3 and build(index=None) == -3
    assert build(dd=100) == -1 and build(rr=0) == -1
    assert build(nbytes=ib - 1) == -4 and build(index=2 * a + 16) == -4
    assert build(flags=2) == -2
    assert build(flags=BF) == -4                                         # the planes do not fit
    assert build(ref=None, dd=100, nbytes=0, flags=2) == -3              # order: NULL first
    assert build(dd=100, nbytes=0, flags=2) == -1                        # then shape
    assert build(nbytes=0, flags=2) == -4                                # then the block, then the flag

    def query(ref=a, index=2 * a, nbytes=ib, qry=3 * a, qq=q, nn=n, dd=d, idx=4 * a, dist=5 * a, unc=6 * a,
              bound=7 * a, ws=8 * a, wbytes=wb, flags=F32):
        return lib.scl_topn_index_query(_p(ref), r, dd, _p(index), nbytes, _p(qry), qq, nn, 0, _p(idx),
                                        _p(dist), _p(unc), _p(bound), _p(ws), wbytes, flags, None)

    for name in ('ref', 'index', 'qry', 'idx', 'dist', 'ws'):
        assert query(**{name: None}) == -3, name
    assert query(unc=None) == -3 and query(bound=None) == -3             # both or neither
    assert query(dd=100) == -1 and query(nn=26) == -1 and query(nn=r + 1) == -1 and query(qq=0) == -1
    assert query(wbytes=wb - 1) == -4 and query(ws=8 * a + 64) == -4
    assert query(nbytes=ib - 1) == -4 and query(index=2 * a + 128) == -4
    assert query(flags=2) == -2
    assert query(qq=33, wbytes=0) == -4                                  # the scan route sizes its own
    assert query(unc=None, dd=100, wbytes=0, flags=2) == -3
    assert query(dd=100, wbytes=0, flags=2) == -1
    assert query(wbytes=0, flags=2) == -4


# ---- Localizer bookkeeping around a NumPy stand-in for the index -------------------------------------
def _numpy_topn(ref_f, query_f, n):
    r64, q64 = np.asarray(ref_f, np.float64), np.asarray(query_f, np.float64)
    d2 = ((q64[:, None, :] - r64[None]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :n]
    return np.sqrt(np.take_along_axis(d2, idx, 1)), idx


def _torch_topn(ref, query, n, idx_offset=0, score='f32', certify=True, stats=None):
    d, i = _numpy_topn(ref.numpy(), query.numpy(), n)
    return torch.from_numpy(d), torch.from_numpy(i)


def _track(m=120, q=23, e=24, seed=5):
    """References along a track 0.5 m apart (thinning at 1.2 m drops most of them), queries near it."""
    rng = np.random.default_rng(seed)
    ref_xy = np.stack([0.5 * np.arange(m), 0.1 * rng.standard_normal(m)], 1)
    qry_xy = np.stack([rng.uniform(0, 0.5 * m, q), rng.standard_normal(q)], 1)
    ref_f = rng.standard_normal((m, e)).astype(np.float32)
    qry_f = rng.standard_normal((q, e)).astype(np.float32)
    return ref_xy, qry_xy, ref_f, qry_f


def _assert_payload_equal(a, b):
    assert len(a) == len(b) == 6
    np.testing.assert_array_equal(np.asarray(a[0]), np.asarray(b[0]))
    np.testing.assert_array_equal(np.asarray(a[1]), np.asarray(b[1]))
    np.testing.assert_array_equal(np.asarray(a[2]), np.asarray(b[2]))
    assert list(a[3]) == list(b[3])
    np.testing.assert_array_equal(np.asarray(a[4]), np.asarray(b[4]))
    assert list(a[5]) == list(b[5])


@pytest.mark.parametrize("l", [0.0, 1.2])
def test_localizer_bookkeeping_matches_retrieve(monkeypatch, l):
    from sklearn.metrics import pairwise_distances
    from soft_contrastive_learning_amd.evaluation import localize, retrieval, top_n
    ref_xy, qry_xy, ref_f, qry_f = _track()
    loc = localize.Localizer(ref_f, ref_xy, n=5, l=l, query_fn=_numpy_topn)
    if l > 0:
        assert len(loc.ref_idx) < len(ref_xy) // 2                       # the thinning thins
    idx, fd, xy = loc.locate_descriptors(qry_f)
    assert idx.shape == (23, 5) and fd.shape == (23, 5) and fd.dtype == np.float64 and xy.shape == (23, 5, 2)
    # original indices: the hits are rows of the FULL list, and only surviving ones
    assert set(idx.ravel().tolist()) <= set(loc.ref_idx)
    want_d = np.sqrt(((qry_f.astype(np.float64)[:, None, :] - ref_f.astype(np.float64)[idx]) ** 2).sum(-1))
    np.testing.assert_allclose(fd, want_d, rtol=1e-12)
    np.testing.assert_array_equal(xy, ref_xy[idx])
    # the payload of top_n.retrieve on the same stand-in
    monkeypatch.setattr(retrieval, 'topn_l2', _torch_topn)
    full = pairwise_distances(qry_xy, ref_xy, metric='euclidean')
    want = top_n.retrieve(torch.from_numpy(ref_f), torch.from_numpy(qry_f), full, ref_xy, 5, l, 'f32')
    _assert_payload_equal(localize.localize_set(loc, qry_f, full, batch=4), want)
    np.testing.assert_array_equal(np.asarray(want[0]), idx)
    with pytest.raises(ValueError):
        localize.Localizer(ref_f, ref_xy, n=5, l=1000.0, query_fn=_numpy_topn)


def test_command_batches_give_the_same_pickle(tmp_path):
    from soft_contrastive_learning_amd.evaluation import localize, top_n
    from soft_contrastive_learning_amd.util import io
    ref_xy, qry_xy, ref_f, qry_f = _track()
    for name, f in (('ref', ref_f), ('query', qry_f), ('pca', ref_f)):
        io.save_pickle([row for row in f], str(tmp_path / ('set_%s.v1.pickle' % name)))
    for name, xy in (('ref', ref_xy), ('query', qry_xy)):
        io.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]],
                     'northing': [repr(float(v)) for v in xy[:, 1]]}, str(tmp_path / ('%s.csv' % name)))
    payloads = []
    for batch in (1, 7):
        out_root = str(tmp_path / ('out%d' % batch))
        argv = ['--pca_lv_pickle', str(tmp_path / 'set_pca.v1.pickle'),
                '--query_lv_pickle', str(tmp_path / 'set_query.v1.pickle'),
                '--ref_lv_pickle', str(tmp_path / 'set_ref.v1.pickle'),
                '--query_csv', str(tmp_path / 'query.csv'), '--ref_csv', str(tmp_path / 'ref.csv'),
                '--N', '5', '--out_root', out_root, '--L', '1.2', '--D', '0', '--batch', str(batch)]
        out = localize.main(argv, query_fn=_numpy_topn)
        assert out == top_n.out_pickle_path(out_root, str(tmp_path / 'set_query.v1.pickle'), 1.2, 0)
        assert os.path.exists(out)
        payloads.append(io.load_pickle(out))
    _assert_payload_equal(payloads[0], payloads[1])
    assert len(payloads[0][0]) == 23 and len(payloads[0][0][0]) == 5

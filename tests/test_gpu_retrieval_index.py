"""GPU checks of the prepared retrieval index (csrc/topn.hip: scl_topn_index_build / _query,
evaluation/retrieval.RetrievalIndex) and of the localiser built on it (evaluation/localize.py).

The defining property: ``RetrievalIndex(ref, off, score).query(q, n)`` equals
``retrieval.topn_l2(ref, q, n, off, score)`` in both tensors — and, so that the exact fallback
cannot hide a broken scan, no query of the tie-free sets below may need it."""
import functools
import os

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


def _both(dev, ref, qry, n, score='f32', idx_offset=0):
    """(index result, index stats, topn_l2 result, topn_l2 stats) on the same operands."""
    from soft_contrastive_learning_amd.evaluation import retrieval
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    si, sl = {}, {}
    got = retrieval.RetrievalIndex(rt, idx_offset, score).query(qt, n, stats=si)
    want = retrieval.topn_l2(rt, qt, n, idx_offset, score, stats=sl)
    return got, si, want, sl


STREAM_SHAPES = [(25, 1, 32, 25),            # R <= KEEP: everything nominated
                 (33, 1, 32, 25),            # one row past a tile
                 (1000, 5, 64, 25),
                 (4099, 32, 256, 25),        # ragged last tile, full query tile
                 (4099, 32, 128, 1),
                 (900, 20, 40, 7),           # padded to 64
                 (700, 3, 96, 25),           # padded to 128
                 (40000, 1, 32, 25),         # many workgroups, above the threshold scheme's 32 768
                 (40000, 32, 256, 25),
                 (100003, 8, 128, 7)]


@pytest.mark.parametrize("r,q,d,n", STREAM_SHAPES)
def test_stream_route_matches_kdtree_and_topn_l2(dev, r, q, d, n):
    ref, qry = U.retrieval_sets(r, q, d)
    want_d, want_i = TN.topn_kdtree(ref, qry, n)
    (got_d, got_i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, n)
    assert st['route'] == 'stream'
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
    np.testing.assert_allclose(got_d.cpu().numpy(), want_d, rtol=1e-12, atol=0)
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)
    # the fallback cap: on these inputs the gap between the 32nd and the n-th squared distance is
    # at least 13 x the certificate's eps, so the scan alone must have produced the lists
    assert st['uncertified'] == 0, st


@pytest.mark.parametrize("score", ['f32', 'bf16x3'])
@pytest.mark.parametrize("q,r,d", [(33, 1000, 128), (70, 32768, 64), (130, 5000, 256)])
def test_scan_route_equals_topn_l2(dev, q, r, d, score):
    ref, qry = U.retrieval_sets(r, q, d)
    (got_d, got_i), st, (l2_d, l2_i), sl = _both(dev, ref, qry, 25, score)
    assert st['route'] == 'scan'
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)
    assert st['uncertified'] == sl['uncertified']


@pytest.mark.parametrize("score", ['f32', 'bf16x3'])
def test_ties_and_offset(dev, score):
    ref, qry = U.retrieval_sets(300, 10, 64)
    ref[150] = ref[3]          # exact tie: lower index first
    qry[0] = ref[3]
    (d, i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, 5, score, idx_offset=1000)
    assert st['route'] == 'stream'
    assert list(i[0, :2].cpu().numpy()) == [1003, 1150]
    assert float(d[0, 0]) == 0.0 and float(d[0, 1]) == 0.0
    assert int(i.min()) >= 1000
    assert torch.equal(i, l2_i) and torch.equal(d, l2_d)


def test_many_equal_scores_behind_the_top_n(dev):
    """400 exact duplicates at rank 26 and beyond: more equal scores than the selection's
    pre-filter passes on, so the step runs on all of its slots — and since the 25 nearest are
    well separated from them (0.1 in distance, the duplicates 2.5 further), nothing may be
    handed to the exact fallback."""
    rng = np.random.default_rng(9)
    d = 64

    def unit(m):
        v = rng.standard_normal((m, d))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    q = rng.standard_normal((1, d))
    near = q + 0.1 * np.arange(1, 26)[:, None] * unit(25)
    dup = np.repeat(q + 5.0 * unit(1), 400, axis=0)
    far = q + rng.uniform(8.0, 9.0, (575, 1)) * unit(575)
    perm = rng.permutation(1000)
    ref = np.concatenate([near, dup, far])[perm].astype(np.float32)
    qry = q.astype(np.float32)
    want_d, want_i = TN.topn_kdtree(ref, qry, 25)
    assert sorted(perm[want_i[0]].tolist()) == list(range(25))       # the 25 near rows
    (got_d, got_i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, 25)
    assert st['route'] == 'stream' and st['uncertified'] == 0, st
    np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
    np.testing.assert_allclose(got_d.cpu().numpy(), want_d, rtol=1e-12, atol=0)
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)


def test_near_duplicate_clusters(dev):
    """The construction of test_gpu_topn.test_topn_certificate_resolves_near_duplicate_clusters, its
    40 queries cut to the first 32: the two clustered queries must be flagged and resolved exactly."""
    rng = np.random.default_rng(123)
    r, q, d, n = 6000, 40, 128, 25
    ref = rng.standard_normal((r, d)).astype(np.float32)
    qry = rng.standard_normal((q, d)).astype(np.float32)
    rows_a = rng.permutation(r)[:48]
    ref[rows_a] = qry[3] * (1.0 + 1e-6 * rng.standard_normal((48, 1)).astype(np.float32)) \
        + 1e-6 * rng.standard_normal((48, d)).astype(np.float32)
    rows_b = np.setdiff1d(rng.permutation(r)[:80], rows_a)[:60]
    ref[rows_b] = (qry[7] + 0.01 * rng.standard_normal(d)).astype(np.float32)
    qry = qry[:32]
    want_d, want_i = TN.topn_kdtree(ref, qry, n)
    (got_d, got_i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, n)
    assert st['route'] == 'stream'
    assert 2 <= st['uncertified'] <= 6, st
    gi = got_i.cpu().numpy()
    np.testing.assert_array_equal(gi[3], want_i[3])
    assert list(gi[7]) == np.sort(rows_b)[:n].tolist()
    ok = np.ones(32, bool)
    ok[7] = False                                   # (the tree may order exact ties differently)
    np.testing.assert_array_equal(gi[ok], want_i[ok])
    np.testing.assert_allclose(got_d.cpu().numpy(), want_d, rtol=1e-12, atol=1e-300)
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)


def test_no_state_between_calls(dev):
    from soft_contrastive_learning_amd.evaluation import retrieval
    ref, qry = U.retrieval_sets(5000, 33, 128)
    ref2, _ = U.retrieval_sets(3000, 1, 128, seed_r=21)
    rt, qt, rt2 = (torch.tensor(a, device=dev) for a in (ref, qry, ref2))
    one = retrieval.RetrievalIndex(rt)
    first = one.query(qt[:32], 25)
    one.query(qt[:1], 25)
    wide = one.query(qt, 25)
    last = one.query(qt[:32], 25)
    assert torch.equal(first[0], last[0]) and torch.equal(first[1], last[1])
    assert torch.equal(wide[1][:32], first[1])
    # two indexes over different sets, queried alternately
    other = retrieval.RetrievalIndex(rt2)
    alone_a, alone_b = one.query(qt[:8], 25), other.query(qt[:8], 25)
    for _ in range(2):
        a, b = one.query(qt[:8], 25), other.query(qt[:8], 25)
        assert torch.equal(a[0], alone_a[0]) and torch.equal(a[1], alone_a[1])
        assert torch.equal(b[0], alone_b[0]) and torch.equal(b[1], alone_b[1])
    assert not torch.equal(alone_a[1], alone_b[1])


def test_delegated_shapes_equal_topn_l2(dev):
    """What the index does not cover goes to topn_l2 on the stored rows: n > 25, d > 256."""
    ref, qry = U.retrieval_sets(600, 4, 48)
    (got_d, got_i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, 30)
    assert st['route'] == 'delegate'
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)
    ref, qry = U.retrieval_sets(300, 3, 520)
    (got_d, got_i), st, (l2_d, l2_i), _ = _both(dev, ref, qry, 5)
    assert st['route'] == 'delegate'
    assert torch.equal(got_i, l2_i) and torch.equal(got_d, l2_d)


def _descriptors(m, e, seed):
    """Unit-norm rows with a decaying spectrum, like NetVLAD descriptors."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, e)).astype(np.float32) * np.linspace(1.0, 0.2, e, dtype=np.float32)
    x += 0.5 * rng.standard_normal((m, 1)).astype(np.float32) * rng.standard_normal((1, e)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_row_wise_whitening(dev):
    from soft_contrastive_learning_amd.evaluation.pca import PCAWhitening
    x = _descriptors(300, 32768, 3)
    pca = PCAWhitening(256, device=dev).fit(x)
    batch = pca.transform_rows(x[:7])
    alone = pca.transform_rows(x[:1])
    assert batch.shape == (7, 256) and batch.dtype == torch.float32
    assert torch.equal(alone[0], batch[0])
    want = pca.transform(x[:7])
    rel = float((batch - want).abs().max() / want.abs().max())
    print('transform_rows vs transform: max abs difference / max abs value = %.3g' % rel)
    assert rel <= 1e-5, rel


def _track(m, q, seed=5):
    rng = np.random.default_rng(seed)
    ref_xy = np.stack([0.5 * np.arange(m), 0.1 * rng.standard_normal(m)], 1)
    qry_xy = np.stack([rng.uniform(0, 0.5 * m, q), rng.standard_normal(q)], 1)
    return ref_xy, qry_xy


def _assert_payload_equal(a, b, rtol=0.0):
    assert len(a) == len(b) == 6
    np.testing.assert_array_equal(np.asarray(a[0]), np.asarray(b[0]))
    np.testing.assert_array_equal(np.asarray(a[1]), np.asarray(b[1]))
    np.testing.assert_allclose(np.asarray(a[2]), np.asarray(b[2]), rtol=rtol, atol=0)
    assert list(a[3]) == list(b[3])
    np.testing.assert_array_equal(np.asarray(a[4]), np.asarray(b[4]))
    assert list(a[5]) == list(b[5])


@pytest.mark.parametrize("l", [0.0, 1.2])
def test_locate_descriptors_equals_retrieve(dev, l):
    from sklearn.metrics import pairwise_distances
    from soft_contrastive_learning_amd.evaluation import localize, top_n
    ref_xy, qry_xy = _track(400, 37)
    ref_f, qry_f = U.retrieval_sets(400, 37, 64)
    full = pairwise_distances(qry_xy, ref_xy, metric='euclidean')
    loc = localize.Localizer(ref_f, ref_xy, n=5, l=l, device=dev)
    if l > 0:
        assert len(loc.ref_idx) < 200
    want = top_n.retrieve(torch.tensor(ref_f, device=dev), torch.tensor(qry_f, device=dev), full, ref_xy,
                          5, l, 'f32')
    _assert_payload_equal(localize.localize_set(loc, qry_f, full, batch=7), want)
    idx, fd, xy = loc.locate_descriptors(qry_f[:3])
    np.testing.assert_array_equal(idx, np.asarray(want[0])[:3])
    np.testing.assert_array_equal(fd, np.asarray(want[2])[:3])
    np.testing.assert_array_equal(xy, ref_xy[idx])


def test_locate_descriptors_with_pca(dev):
    from sklearn.metrics import pairwise_distances
    from soft_contrastive_learning_amd.evaluation import localize, top_n
    from soft_contrastive_learning_amd.evaluation.pca import PCAWhitening
    ref_xy, qry_xy = _track(200, 20)
    pca_f, ref_f, qry_f = _descriptors(300, 2048, 1), _descriptors(200, 2048, 2), _descriptors(20, 2048, 4)
    pca = PCAWhitening(64, device=dev).fit(pca_f)
    full = pairwise_distances(qry_xy, ref_xy, metric='euclidean')
    loc = localize.Localizer(ref_f, ref_xy, pca=pca, n=5, l=0.0, device=dev)
    want = top_n.retrieve(pca.transform(ref_f), pca.transform(qry_f), full, ref_xy, 5, 0.0, 'f32')
    _assert_payload_equal(localize.localize_set(loc, qry_f, full, batch=1), want, rtol=1e-5)


def test_locate_images(dev):
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.evaluation.inference import extract_features
    from soft_contrastive_learning_amd.model import nets
    model = nets.VGG16NetVLAD().to(dev).eval()
    imgs = U.pose_images(50, 64, 80)
    feats = extract_features(model, lambda i: imgs[i], 50, images_per_pass=10, device=dev, loader_threads=1)
    ref_xy, _ = _track(50, 1)
    loc = localize.Localizer(np.stack(feats), ref_xy, model=model, n=3, device=dev)
    idx, fd, xy = loc.locate(imgs[:4])
    assert idx.shape == (4, 3) and xy.shape == (4, 3, 2)
    assert list(idx[:, 0]) == [0, 1, 2, 3]
    assert float(fd[:, 0].max()) < 1e-3, fd[:, 0]
    # (l = 0 lists reference 0 twice, evaluation/top-n.py:91-94: frame 0's runner-up is itself)
    assert list(idx[0, :2]) == [0, 0] and float(fd[1:, 1].min()) > 1e-3
    np.testing.assert_array_equal(xy[:, 0], ref_xy[:4])


def test_command_writes_top_n_mains_pickle(dev, tmp_path, monkeypatch, capsys):
    from soft_contrastive_learning_amd.evaluation import localize, top_n
    from soft_contrastive_learning_amd.util import io
    ref_xy, qry_xy = _track(300, 19)
    ref_f, qry_f = U.retrieval_sets(300, 19, 64)
    for name, f in (('ref', ref_f), ('query', qry_f), ('pca', ref_f)):
        io.save_pickle([row for row in f], str(tmp_path / ('set_%s.v1.pickle' % name)))
    for name, xy in (('ref', ref_xy), ('query', qry_xy)):
        io.save_csv({'easting': [repr(float(v)) for v in xy[:, 0]],
                     'northing': [repr(float(v)) for v in xy[:, 1]]}, str(tmp_path / ('%s.csv' % name)))

    def argv(out):
        return ['--pca_lv_pickle', str(tmp_path / 'set_pca.v1.pickle'),
                '--query_lv_pickle', str(tmp_path / 'set_query.v1.pickle'),
                '--ref_lv_pickle', str(tmp_path / 'set_ref.v1.pickle'),
                '--query_csv', str(tmp_path / 'query.csv'), '--ref_csv', str(tmp_path / 'ref.csv'),
                '--N', '25', '--out_root', str(tmp_path / out), '--L', '1.2', '--D', '0']
    got = localize.main(argv('loc') + ['--batch', '4'])
    assert 'queries/s' in capsys.readouterr().out
    # top_n.main has no "no whitening" of its own: D = 0 passes the descriptors through
    monkeypatch.setattr(top_n, 'whiten', lambda pca_f, sets, d, device, backend: [
        torch.tensor(np.asarray(f, dtype=np.float32), device=device) for f in sets])
    want = top_n.main(argv('top'))
    assert len(want) == 1
    assert os.path.relpath(got, str(tmp_path / 'loc')) == os.path.relpath(want[0], str(tmp_path / 'top'))
    _assert_payload_equal(io.load_pickle(got), io.load_pickle(want[0]))


# ---- the workspace and index-block layouts, between guard bands ----------------------------------------
# Every C entry point below gets EXACTLY the bytes its size query returned, inside a larger buffer whose
# 4096 bytes on either side must come back untouched; the lists must be the oracle's with nothing handed
# to the exact fallback (the entry points are called directly: there is none), and a run on a buffer
# full of 0xA5 must equal a run on a zeroed one — nothing is read before it is written.
F32, BF = 0, 1    # (the bands: tests/util_guard.py)


@functools.lru_cache(maxsize=None)
def _guard_sets(r, q, n=5):
    """(ref, qry, oracle dists, oracle idx) at d = 32, computed once and shared read-only."""
    ref, qry = U.retrieval_sets(r, q, 32)
    out = (ref, qry) + TN.topn_kdtree(ref, qry, n)
    for a in out:
        a.setflags(write=False)
    return out


def _outputs(dev, q, n, certify=True):
    idx = torch.full((q, n), -7, dtype=torch.int64, device=dev)
    dist = torch.full((q, n), -1.0, dtype=torch.float64, device=dev)
    flag = torch.ones(q, dtype=torch.uint8, device=dev) if certify else None
    bound = torch.full((q,), -1.0, dtype=torch.float64, device=dev) if certify else None
    return idx, dist, flag, bound


def _assert_oracle_lists(out, want_d, want_i):
    idx, dist, flag, _ = out
    if flag is not None:
        assert int(flag.sum()) == 0, flag
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_allclose(dist.cpu().numpy(), want_d, rtol=1e-12, atol=0)


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


def _cert_between_bands(dev, r, q, flags, certify, fill, n=5):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    ref, qry, want_d, want_i = _guard_sets(r, q)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    ws = _Guarded(dev, lib.scl_topn_l2_ex_workspace_bytes(r, q, 32, n, flags), fill)
    out = _outputs(dev, q, n, certify)
    L.check(lib.scl_topn_l2_cert(L.ptr(rt), r, L.ptr(qt), q, 32, n, 0, L.ptr(out[0]), L.ptr(out[1]),
                                 L.ptr(out[2]), L.ptr(out[3]), L.ptr(ws.inner), ws.inner.numel(), flags,
                                 L.stream_of(rt)))
    ws.assert_bands_intact()
    _assert_oracle_lists(out, want_d, want_i)
    return out


# 1000: the sorted-list scan, refnorm[R] not a multiple of 64 floats.  32771: just above the 32768 from
# which a certified call uses the threshold scheme's layout (pre | cs | ci | tau | cnt).
@pytest.mark.parametrize("flags", [F32, BF])
@pytest.mark.parametrize("r,q", [(1000, 33), (32771, 40)])
def test_one_shot_workspace_between_guard_bands(dev, r, q, flags):
    _assert_same(_cert_between_bands(dev, r, q, flags, True, FILL),
                 _cert_between_bands(dev, r, q, flags, True, 0))


def test_one_shot_workspace_between_guard_bands_without_certificate(dev):
    _assert_same(_cert_between_bands(dev, 1000, 33, BF, False, FILL),
                 _cert_between_bands(dev, 1000, 33, BF, False, 0))


def _index_between_bands(dev, flags, fill, r=32771, n=5):
    """scl_topn_index_build into a guarded block, then a stream (Q = 8) and a scan (Q = 40) query of it,
    each with a guarded workspace."""
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    ref, qry, want_d, want_i = _guard_sets(r, 40)
    rt, qt = torch.tensor(ref, device=dev), torch.tensor(qry, device=dev)
    index = _Guarded(dev, lib.scl_topn_index_bytes(r, 32, flags), fill)
    L.check(lib.scl_topn_index_build(L.ptr(rt), r, 32, L.ptr(index.inner), index.inner.numel(), flags,
                                     L.stream_of(rt)))
    index.assert_bands_intact()
    outs = []
    for q in (8, 40):
        ws = _Guarded(dev, lib.scl_topn_index_query_workspace_bytes(r, q, 32, n, flags), fill)
        out = _outputs(dev, q, n)
        L.check(lib.scl_topn_index_query(L.ptr(rt), r, 32, L.ptr(index.inner), index.inner.numel(), L.ptr(qt), q,
                                         n, 0, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]),
                                         L.ptr(ws.inner), ws.inner.numel(), flags, L.stream_of(rt)))
        ws.assert_bands_intact()
        index.assert_bands_intact()
        _assert_oracle_lists(out, want_d[:q], want_i[:q])
        outs += out
    return outs


@pytest.mark.parametrize("flags", [F32, BF])
def test_index_block_and_query_workspaces_between_guard_bands(dev, flags):
    _assert_same(_index_between_bands(dev, flags, FILL), _index_between_bands(dev, flags, 0))

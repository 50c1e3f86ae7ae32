"""Host side of the wrd / prodwrd / sumwrd losses: the sampler's 'wrd' payload against the
reference's own get_tuple (tests/golden/golden_ref_wrd_v1.json), the trainer's dispatch, and the
C-ABI surface.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import util_data as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'golden_ref_wrd_v1.json')))


def test_wrd_payload_equals_the_reference_get_tuple(golden):
    from soft_contrastive_learning_amd.train import sampler as S
    xy, yaw = U.sampler_dataset()
    assert len(golden['sampler']) >= 3
    for c in golden['sampler']:
        p, n = c['tuple_shape'][1], c['tuple_shape'][2]
        sm = S.TupleSampler(xy, yaw, p, n, distance_type='wrd', rng=np.random.RandomState(c['seed']),
                            alpha=c['alpha'], beta=c['beta'])
        distances, indices = sm.get_tuple(c['anchors'], c['tuple_shape'])
        assert [int(i) for i in indices] == c['indices'], c['name']
        got, want = np.asarray(distances, dtype=np.float64), np.asarray(c['distances'])
        assert got.shape == want.shape == (len(c['anchors']), 2 * (p + n))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=c['name'])
        # positive-side weights first: near 1 for the positives, near 0 for the negatives
        assert (got[:, :p] > 0.5).all() and (got[:, p:p + n] <= 0.5).all()


def test_wrd_payload_defaults_are_the_reference_flags(golden):
    from soft_contrastive_learning_amd.train import sampler as S
    xy, yaw = U.sampler_dataset()
    c = golden['sampler'][0]
    assert (c['alpha'], c['beta']) == (0.8, 15)
    sm = S.TupleSampler(xy, yaw, 12, 12, distance_type='wrd', rng=np.random.RandomState(c['seed']))
    distances, _ = sm.get_tuple(c['anchors'], c['tuple_shape'])
    np.testing.assert_allclose(np.asarray(distances), np.asarray(c['distances']), rtol=1e-12, atol=0)


def test_swrd_payload_is_still_refused():
    from soft_contrastive_learning_amd.train import sampler as S
    xy, yaw = U.sampler_dataset()
    with pytest.raises(ValueError):
        S.TupleSampler(xy, yaw, distance_type='swrd')


@pytest.mark.parametrize('loss', ['wrd', 'prodwrd', 'sumwrd'])
def test_compute_loss_splits_the_payload_like_the_reference(monkeypatch, loss):
    """train/train.py:677-681: [T, 2(P+N)] -> reshape [T, 2(P+N), 1] -> split in two along axis 1;
    :842-849: anchor, positives, negatives, the two weight tensors and margin_1, nothing else."""
    from soft_contrastive_learning_amd.model import losses
    from soft_contrastive_learning_amd.train import train as T
    t, p, n, e = 2, 3, 4, 8
    flags = T.make_parser().parse_args(['--loss', loss, '--tuples_per_batch', str(t), '--margin_1', '0.25',
                                        '--positives_per_tuple', str(p), '--negatives_per_tuple', str(n)])
    assert loss in T.SUPPORTED_LOSSES
    out = torch.arange(t * (1 + p + n) * e, dtype=torch.float32).reshape(t * (1 + p + n), e)
    payload = torch.arange(t * 2 * (p + n), dtype=torch.float32).reshape(t, 2 * (p + n))
    seen = {}

    def stub(*args, **kwargs):
        seen['args'], seen['kwargs'] = args, kwargs
        return torch.zeros(())
    for name in ('wrd_loss', 'prodwrd_loss', 'sumwrd_loss'):
        monkeypatch.setattr(losses, name, stub if name == loss + '_loss' else None)
    T.compute_loss(flags, T.tuple_shape_for(loss, p, n), out, payload)
    a, pos, neg, pw, nw, margin = seen['args']
    assert seen['kwargs'] == {} and margin == 0.25
    rows = out.reshape(t, 1 + p + n, e)
    assert torch.equal(a, rows[:, :1]) and torch.equal(pos, rows[:, 1:1 + p]) and torch.equal(neg, rows[:, 1 + p:])
    assert tuple(pw.shape) == tuple(nw.shape) == (t, p + n, 1)
    assert torch.equal(pw[:, :, 0], payload[:, :p + n]) and torch.equal(nw[:, :, 0], payload[:, p + n:])


def test_compute_loss_still_rejects_the_rest_of_the_family():
    from soft_contrastive_learning_amd.train import train as T
    for loss in ('residual_det', 'swrd'):
        assert loss not in T.SUPPORTED_LOSSES
        flags = T.make_parser().parse_args(['--loss', loss])
        with pytest.raises(ValueError):
            T.compute_loss(flags, [1, 12, 12], torch.zeros(25, 8), torch.zeros(1, 48))


def test_distance_type_and_parser_default():
    from soft_contrastive_learning_amd.train import train as T
    for loss in ('wrd', 'prodwrd', 'sumwrd'):
        assert T.distance_type(loss) == 'wrd'
    assert T.distance_type('swrd') == 'swrd'
    assert T.make_parser().parse_args([]).loss == 'wms'


def test_synthetic_tuples_carry_the_wrd_payload():
    from soft_contrastive_learning_amd.train import train as T
    flags = T.make_parser().parse_args(['--loss', 'sumwrd', '--tuples_per_batch', '2', '--height', '8',
                                        '--width', '8', '--positives_per_tuple', '3',
                                        '--negatives_per_tuple', '5'])
    d, img = T.SyntheticTuples(flags, [1, 3, 5], torch.device('cpu')).batch()
    assert tuple(d.shape) == (2, 16) and d.dtype == torch.float32 and tuple(img.shape) == (18, 8, 8, 3)
    pos_side, neg_side = d[:, :8], d[:, 8:]
    torch.testing.assert_close(pos_side + neg_side, torch.ones(2, 8))      # the two sigmoids
    assert (pos_side[:, :3] >= 0.5).all() and (pos_side[:, 3:] <= 0.5).all()


def test_loss_shape_errors_need_no_device():
    from soft_contrastive_learning_amd.model import losses as M
    a, pos, neg = torch.zeros(2, 1, 16), torch.zeros(2, 4, 16), torch.zeros(2, 4, 16)
    w = torch.ones(2, 8, 1)
    for fn in (M.wrd_loss, M.prodwrd_loss, M.sumwrd_loss):
        with pytest.raises(ValueError):
            fn(a, pos, neg, w, w, 0.1, dimensions=0)
        with pytest.raises(ValueError):
            fn(a, pos, neg, w, w, 0.1, dimensions=9)
        with pytest.raises(ValueError):
            fn(a, pos, neg, torch.ones(2, 7, 1), w, 0.1, dimensions=3)
        with pytest.raises(ValueError):
            fn(a, torch.zeros(2, 20, 16), torch.zeros(2, 13, 16), torch.ones(2, 33, 1), torch.ones(2, 33, 1), 0.1)


def test_header_signatures_and_both_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, 'include', 'scl_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    new = {'scl_spectral_loss_workspace_bytes', 'scl_spectral_loss_fwd'}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    for lib in (_lib.load(), _lib.load(diag=True)):
        assert lib.scl_abi_version() == 12
        for name in new:
            assert getattr(lib, name) is not None
        # pure host functions: sizes and refusals without a device
        assert lib.scl_spectral_loss_workspace_bytes(2, 24, 32768) % 256 == 0
        assert lib.scl_spectral_loss_workspace_bytes(2, 24, 32768) > 0
        assert lib.scl_spectral_loss_workspace_bytes(2, 33, 64) == 0
        assert lib.scl_spectral_loss_fwd(0, None, None, None, 1, 8, 16, 0.1, 3, 2.0, 50.0, 1.0, None, None,
                                         None, None, 0, None) == -3

"""Host side of the eigenvalue / residual losses: the trainer's dispatch for residual_trace,
ntuplet_evmm, ntuplet_trace and ms_sum, the tuple-size refusal, the labels of ms_sum, the Python
validation on CPU tensors and the C-ABI surface of scl_eigen_loss_fwd.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LOSSES = ('residual_trace', 'ntuplet_evmm', 'ntuplet_trace', 'ms_sum')


def reference_labels(t, p, n):
    """train/train.py:830-834, statement by statement."""
    one_batch_classes = np.concatenate((np.zeros(1 + p), np.arange(n) + 1))
    all_labels = one_batch_classes
    for batch in range(1, t):
        all_labels = np.concatenate((all_labels, one_batch_classes + batch * (n + 1)))
    return all_labels


def _flags(loss, t=2, p=3, n=4, extra=()):
    from soft_contrastive_learning_amd.train import train as T
    return T.make_parser().parse_args(['--loss', loss, '--tuples_per_batch', str(t), '--margin_1', '0.25',
                                       '--positives_per_tuple', str(p), '--negatives_per_tuple', str(n)]
                                      + list(extra))


@pytest.mark.parametrize('loss', NEW_LOSSES)
def test_compute_loss_forwards_what_the_reference_forwards(monkeypatch, loss):
    """train/train.py:780-791: anchor, positives, negatives and margin_1, nothing else; :829-837:
    ms_sum also gets the labels, the whole output and ms_mining = the --msmining flag."""
    from soft_contrastive_learning_amd.model import losses
    from soft_contrastive_learning_amd.train import train as T
    t, p, n, e = 2, 3, 4, 8
    flags = _flags(loss, t, p, n)
    assert loss in T.SUPPORTED_LOSSES and T.distance_type(loss) == 'none'
    out = torch.arange(t * (1 + p + n) * e, dtype=torch.float32).reshape(t * (1 + p + n), e)
    labels = torch.as_tensor(reference_labels(t, p, n))
    seen = {}

    def stub(*args, **kwargs):
        seen['args'], seen['kwargs'] = args, kwargs
        return torch.zeros(())
    name = 'ms_sum' if loss == 'ms_sum' else loss + '_loss'
    for other in ('residual_trace_loss', 'ntuplet_evmm_loss', 'ntuplet_trace_loss', 'ms_sum',
                  'residual_det_loss', 'ms_loss'):
        monkeypatch.setattr(losses, other, stub if other == name else None)
    T.compute_loss(flags, T.tuple_shape_for(loss, p, n), out, labels if loss == 'ms_sum' else None)
    rows = out.reshape(t, 1 + p + n, e)
    a, pos, neg, margin = seen['args'][:4]
    assert margin == 0.25
    assert torch.equal(a, rows[:, :1]) and torch.equal(pos, rows[:, 1:1 + p]) and torch.equal(neg, rows[:, 1 + p:])
    if loss == 'ms_sum':
        assert len(seen['args']) == 6 and seen['kwargs'] == {'ms_mining': False}
        assert torch.equal(seen['args'][4], labels) and seen['args'][5] is out
    else:
        assert len(seen['args']) == 4 and seen['kwargs'] == {}


def test_ms_sum_forwards_the_msmining_flag(monkeypatch):
    from soft_contrastive_learning_amd.model import losses
    from soft_contrastive_learning_amd.train import train as T
    flags = _flags('ms_sum', extra=['--msmining', '1'])
    seen = {}
    monkeypatch.setattr(losses, 'ms_sum', lambda *a, **k: seen.update(k) or torch.zeros(()))
    T.compute_loss(flags, [1, 3, 4], torch.zeros(16, 8), torch.zeros(16))
    assert seen == {'ms_mining': True}


def test_ms_sum_is_five_ms_loss_plus_residual_det(monkeypatch):
    """model/losses.py:188-194 with its defaults, on stubbed parts."""
    from soft_contrastive_learning_amd.model import losses
    calls = {}
    monkeypatch.setattr(losses, 'ms_loss', lambda *a: calls.setdefault('ms', a) and torch.tensor(2.0))
    monkeypatch.setattr(losses, 'residual_det_loss', lambda *a: calls.setdefault('det', a) and torch.tensor(0.5))
    got = losses.ms_sum('a', 'p', 'n', 0.1, 'labels', 'emb')
    assert float(got) == 10.5
    assert calls['ms'] == ('labels', 'emb', 2.0, 50.0, 1.0, 0.1, False)
    assert calls['det'] == ('a', 'p', 'n', 0.1, 10)


@pytest.mark.parametrize('t,p,n', [(1, 12, 12), (3, 2, 4)])
def test_ms_sum_labels_are_the_reference_labels(t, p, n):
    from soft_contrastive_learning_amd.train import train as T
    flags = _flags('ms_sum', t, p, n, extra=['--height', '8', '--width', '8'])
    want = reference_labels(t, p, n)
    d, img = T.SyntheticTuples(flags, [1, p, n], torch.device('cpu')).batch()
    assert d.dtype == torch.float64 and tuple(img.shape) == (t * (1 + p + n), 8, 8, 3)
    np.testing.assert_array_equal(d.numpy(), want)
    np.testing.assert_array_equal(T.batch_distances(flags, None, torch.device('cpu')).numpy(), want)
    # ms_loss hands out the same vector
    np.testing.assert_array_equal(
        T.batch_distances(_flags('ms_loss', t, p, n), None, torch.device('cpu')).numpy(), want)
    for loss in ('residual_trace', 'ntuplet_evmm', 'ntuplet_trace'):
        f = _flags(loss, t, p, n, extra=['--height', '8', '--width', '8'])
        assert T.SyntheticTuples(f, [1, p, n], torch.device('cpu')).batch()[0] is None
        assert T.batch_distances(f, None, torch.device('cpu')) is None


def test_the_trainer_refuses_sides_below_ten_rows_and_names_the_flag():
    from soft_contrastive_learning_amd.train import train as T
    for loss in ('residual_trace', 'ms_sum'):
        for flag in ('positives_per_tuple', 'negatives_per_tuple'):
            with pytest.raises(SystemExit) as err:
                T.main(['--loss', loss, '--' + flag, '9'])          # refused before any device work
            assert '--' + flag in str(err.value) and loss in str(err.value)
        T.check_tuple_sizes(_flags(loss, 1, 10, 10))
    for loss in ('ntuplet_evmm', 'ntuplet_trace', 'wms'):
        T.check_tuple_sizes(_flags(loss, 1, 2, 3))                  # no dimensions: any size


def test_the_names_left_for_later_are_refused():
    from soft_contrastive_learning_amd.train import train as T
    for loss in ('residual_det', 'swrd', 'pairwise_distance_neg_eigenvalue',
                 'pairwise_huber_distance_neg_eigenvalue', 'incremental_residual_det', 'incremental_det',
                 'incremental_residual_mm', 'incremental_mm', 'ms_det'):
        assert loss not in T.SUPPORTED_LOSSES
        with pytest.raises(ValueError):
            T.compute_loss(_flags(loss, 1, 12, 12), [1, 12, 12], torch.zeros(25, 8), torch.zeros(1, 48))
        assert loss in T.__doc__ or loss.startswith('incremental_')
    assert 'incremental_*' in T.__doc__


def test_losses_are_exported_with_the_reference_signatures():
    import inspect
    from soft_contrastive_learning_amd.model import losses as M
    want = {'residual_det_loss': ['anchor', 'positives', 'negatives', 'margin', 'dimensions'],
            'residual_trace_loss': ['anchor', 'positives', 'negatives', 'margin', 'dimensions'],
            'swrd_loss': ['anchor', 'positives', 'negatives', 'pos_weights', 'neg_weights', 'margin', 'dimensions'],
            'ntuplet_evmm_loss': ['anchor', 'positives', 'negatives', 'margin'],
            'ntuplet_trace_loss': ['anchor', 'positives', 'negatives', 'margin'],
            'neg_eigenvalue_loss': ['anchor', 'negatives'],
            'ms_sum': ['anchor', 'positives', 'negatives', 'margin', 'labels', 'embeddings', 'alpha', 'beta',
                       'lamb', 'eps', 'ms_mining', 'dimensions']}
    for name, params in want.items():
        assert name in M.__all__
        sig = inspect.signature(getattr(M, name))
        assert list(sig.parameters)[:len(params)] == params, name
        if 'dimensions' in params:
            assert sig.parameters['dimensions'].default == 10
        if name != 'ms_sum':
            assert list(sig.parameters)[len(params):] == ['return_terms']
            assert sig.parameters['return_terms'].default is False
    ms = inspect.signature(M.ms_sum).parameters
    assert [ms[k].default for k in ('alpha', 'beta', 'lamb', 'eps', 'ms_mining')] == [2.0, 50.0, 1.0, 0.1, False]


def test_loss_shape_errors_need_no_device():
    from soft_contrastive_learning_amd.model import losses as M

    def rows(p, n, e=16, t=2):
        return tuple(torch.zeros(t, r, e) for r in (1, p, n))

    for fn in (M.residual_det_loss, M.residual_trace_loss):
        for p, n, k in ((20, 13, 10), (4, 4, 0), (4, 6, 5), (6, 4, 5), (0, 4, 1), (4, 0, 1)):
            with pytest.raises(ValueError):
                fn(*rows(p, n), 0.1, dimensions=k)
    for fn in (M.ntuplet_evmm_loss, M.ntuplet_trace_loss):
        for p, n in ((20, 13), (0, 4), (4, 0)):
            with pytest.raises(ValueError):
                fn(*rows(p, n), 0.1)
        a, pos, neg = rows(4, 4)
        with pytest.raises(ValueError):
            fn(a, pos, neg[:, :, :8], 0.1)
        with pytest.raises(ValueError):
            fn(a, pos[:1], neg, 0.1)
        with pytest.raises(ValueError):
            fn(a[:, 0], pos, neg, 0.1)
    a, pos, neg = rows(4, 5)
    for pw, nw in ((torch.ones(2, 5, 1), torch.ones(2, 5, 1)), (torch.ones(2, 4, 1), torch.ones(2, 4, 1)),
                   (torch.ones(2, 4, 2), torch.ones(2, 5, 1)), (torch.ones(2, 9, 1), torch.ones(2, 9, 1)),
                   (None, None)):
        with pytest.raises(ValueError):
            M.swrd_loss(a, pos, neg, pw, nw, 0.1, dimensions=3)
    with pytest.raises(ValueError):
        M.swrd_loss(a, pos, neg, torch.ones(2, 4), torch.ones(2, 5), 0.1, dimensions=5)
    with pytest.raises(ValueError):
        M.neg_eigenvalue_loss(a, torch.zeros(2, 32, 16))
    with pytest.raises(ValueError):
        M.neg_eigenvalue_loss(a, neg[:, :0])


def test_there_is_no_cpu_fallback():
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.model import losses as M
    a, pos, neg = torch.zeros(2, 1, 16), torch.zeros(2, 4, 16), torch.zeros(2, 5, 16)
    with pytest.raises(_lib.SclError):
        M.residual_det_loss(a, pos, neg, 0.1, dimensions=3)
    with pytest.raises(_lib.SclError):
        M.swrd_loss(a, pos, neg, torch.ones(2, 4), torch.ones(2, 5), 0.1, dimensions=3)
    with pytest.raises(_lib.SclError):
        M.ntuplet_evmm_loss(a, pos, neg, 0.1)
    with pytest.raises(_lib.SclError):
        M.neg_eigenvalue_loss(a, neg)


def test_install_as_learnlarge_resolves_the_new_names(monkeypatch):
    import importlib
    import sys
    import soft_contrastive_learning_amd as pkg
    monkeypatch.setattr(sys, 'modules', dict(sys.modules))      # the aliases go with the test
    pkg.install_as_learnlarge()
    mod = importlib.import_module('learnlarge.model.losses')
    for name in ('residual_det_loss', 'residual_trace_loss', 'swrd_loss', 'ntuplet_evmm_loss',
                 'ntuplet_trace_loss', 'neg_eigenvalue_loss', 'ms_sum'):
        assert callable(getattr(mod, name))


def test_header_signatures_and_both_libraries_agree():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, 'include', 'scl_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    new = {'scl_eigen_loss_workspace_bytes', 'scl_eigen_loss_fwd'}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    kinds = dict(re.findall(r"#define SCL_EIGEN_([A-Z_]+) (\d+)", src))
    assert {k: int(v) for k, v in kinds.items()} == {
        'RESIDUAL_DET': _lib.EIGEN_RESIDUAL_DET, 'RESIDUAL_TRACE': _lib.EIGEN_RESIDUAL_TRACE,
        'SWRD': _lib.EIGEN_SWRD, 'NTUPLET_EVMM': _lib.EIGEN_NTUPLET_EVMM,
        'NTUPLET_TRACE': _lib.EIGEN_NTUPLET_TRACE, 'NEG_EIGENVALUE': _lib.EIGEN_NEG_EIGENVALUE}
    assert sorted(int(v) for v in kinds.values()) == list(range(6))
    for lib in (_lib.load(), _lib.load(diag=True)):
        assert lib.scl_abi_version() == 12
        for name in new:
            assert getattr(lib, name) is not None
    # the new kernels are product kernels, not variants
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH):
        blob = open(path, 'rb').read()
        assert b'eigen_solve_kernel' in blob and b'eigen_finish_kernel' in blob


def test_c_abi_validates_on_the_host():
    """Sizes and refusals are pure host work: every call below returns before any launch (the
    pointers are host memory and are never dereferenced)."""
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    raw = ctypes.create_string_buffer(1 << 12)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    for lib in (_lib.load(), _lib.load(diag=True)):
        size = lib.scl_eigen_loss_workspace_bytes
        nb = size(1, 4, 4, 16)
        assert nb > 0 and nb % 256 == 0
        assert size(2, 12, 12, 32768) == lib.scl_spectral_loss_workspace_bytes(2, 24, 32768)
        assert size(2, 16, 16, 96) > 0 and size(2, 17, 16, 96) == 0 and size(2, 31, 1, 96) > 0
        assert size(0, 4, 4, 16) == 0 and size(1, 4, 0, 16) == 0 and size(1, -1, 4, 16) == 0
        assert size(1, 4, 4, 0) == 0
        assert size(1, 0, 31, 16) > 0 and size(1, 0, 32, 16) == 0     # neg_eigenvalue: [anchor; negatives]
        # kind, z, pos_w, neg_w, T, P, N, E, margin, dimensions, loss, terms, coef, workspace, bytes, stream
        ok = (0, p, None, None, 1, 4, 4, 16, 0.1, 3, p, p, None, p, nb, None)

        def with_(**kw):
            a = list(ok)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return lib.scl_eigen_loss_fwd(*a)

        for i in (1, 10, 11, 13):                              # z, loss, terms, workspace
            assert with_(**{'a%d' % i: None}) == -3
        assert with_(a0=2) == -3                                # swrd without weights
        assert with_(a0=2, a2=p) == -3 and with_(a0=2, a3=p) == -3
        assert with_(a0=6) == -2 and with_(a0=-1) == -2         # kind
        assert with_(a4=0) == -1 and with_(a7=0) == -1          # T, E
        assert with_(a5=0) == -1 and with_(a6=0) == -1          # P, N
        assert with_(a5=17, a6=16) == -1                        # P + N = 33
        assert with_(a9=0) == -1 and with_(a9=5) == -1          # dimensions outside 1..min(P, N)
        assert with_(a5=6, a9=5) == -1 and with_(a6=6, a9=5) == -1
        for kind in (1, 2):
            assert with_(a0=kind, a2=p, a3=p, a9=5) == -1
        assert with_(a0=5, a5=0, a6=32) == -1                   # neg_eigenvalue: 33 rows
        for kind in (0, 1, 3, 4):
            assert with_(a0=kind, a5=0) == -1                   # P = 0 is neg_eigenvalue's alone
        assert with_(a14=nb - 1) == -4
        assert with_(a13=ctypes.c_void_p(p.value + 8)) == -4    # misaligned
        # the kinds without `dimensions` ignore it: they get as far as the workspace check
        for kind in (3, 4, 5):
            assert with_(a0=kind, a9=0, a14=nb - 1) == -4
        assert with_(a0=5, a5=0, a14=0) == -4
        # scl_spectral_loss_fwd still takes its own three kinds only
        assert lib.scl_spectral_loss_fwd(3, p, p, p, 1, 8, 16, 0.1, 3, 2.0, 50.0, 1.0, p, p, None, p, 1 << 20,
                                         None) == -2

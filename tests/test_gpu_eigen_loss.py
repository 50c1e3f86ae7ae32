"""GPU parity of the eigenvalue and residual losses (eigen_solve_kernel of csrc/spectral_loss.hip:
residual_det, residual_trace, swrd, ntuplet_evmm, ntuplet_trace, neg_eigenvalue, and ms_sum on top)
against the float64 restatement of the reference in tests/eigen_data.py.

Gates (the project's own, tests/test_gpu_spectral_loss.py): every per-tuple term within 1e-4
relative, the loss within 1e-4 relative + 1e-8, the gradients of anchor, positives and negatives
within GRAD_REL = 2e-4 norm-relative.  Every case asserts on its ORACLE that it is well posed
(eigen_data.assert_well_posed) and, for the hinge losses, that tuples on both sides of the hinge
occur with arguments away from the tie.

Hinge margins: on clustered unit rows lambda_min(pos) - lambda_max(neg) is -4.6 .. -15.7, so with
the reference's margin of 0.1 the loss is identically 0.  For T >= 2 the margin is
eigen_data.hinge_margin of the oracle's raw arguments (one tuple active, one inactive); the T = 1
shape runs once active and once inactive.  ntuplet_trace runs on eigen_data.scale_rows.

Cross-check of the matrix construction: residual_det / swrd against wrd_loss with indicator /
zero-padded weights.  Both are float64 solves of the same Gram entries with different matrix
sizes and rotation orders, so not bit-equal; 1e-9 relative is five orders inside the parity gate
and far above what the Jacobi tolerance leaves — a miss means one of the two builds the wrong matrix.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import eigen_data as ED
from tests import spectral_data as D

pytestmark = pytest.mark.gpu

REL = 1e-4
GRAD_REL = 2e-4
CROSS_REL = 1e-9
MARGIN = 0.1
SEED = 5
# (T, P, N, E, dimensions)
SHAPES = [(2, 4, 4, 64, 3),
          (3, 5, 7, 200, 4),            # odd sizes, E not a multiple of 64
          (4, 3, 6, 48, 3),             # k = P
          (2, 12, 12, 512, 10),         # two E slices
          (2, 12, 12, 512, 12),         # k = P = N
          (1, 12, 12, 32768, 10),       # the trainer's shape
          (2, 16, 16, 96, 16)]          # the S = 32 cap: side matrices of 16 and 17 rows
SHAPE_ID = lambda s: 'T%d_P%d_N%d_E%d_k%d' % s     # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def inputs(kind, shape):
    """z and the swrd weights pos_w[:, :P], neg_w[:, P:] of spectral_data.tuples(..., seed=5)."""
    t, p, n, e, _ = shape
    z, pw, nw = D.tuples(t, p, n, e, SEED)
    if kind == 'ntuplet_trace':
        z = ED.scale_rows(z, SEED)
    return z, np.ascontiguousarray(pw[:, :p]), np.ascontiguousarray(nw[:, p:])


_ORACLE = {}


def oracle(kind, shape, active=True):
    """The float64 reference of a case, computed once and frozen.  ``active`` picks the side of the
    hinge for the T = 1 shape (ignored otherwise)."""
    key = (kind, shape, active)
    if key not in _ORACLE:
        t, p, n, e, k = shape
        z, pw, nw = inputs(kind, shape)
        margin = MARGIN
        if kind in ED.HINGE:
            terms = ED.reference_f64(kind, z, p, 0.0)[1]
            raw = terms[:, 0] - terms[:, 1]
            if t >= 2:
                margin = ED.hinge_margin(raw)
            else:
                margin = float(np.float32(-raw[0] + (1.0 if active else -1.0)))
            args = margin + raw
            floor = 1e-5 if kind == 'ntuplet_evmm' else 1e-3
            assert np.abs(args).min() >= floor, args
            if t >= 2:
                assert (args > 0).any() and (args < 0).any(), args
        loss, terms, grad, spectra = ED.reference_f64(kind, z, p, margin, k, pw, nw)
        ED.assert_well_posed(kind, spectra, k)
        for a in (z, pw, nw, terms, grad):
            a.setflags(write=False)
        _ORACLE[key] = dict(z=z, pw=pw, nw=nw, margin=margin, loss=loss, terms=terms, grad=grad)
    return _ORACLE[key]


def run(kind, z, pw, nw, p, k, dev, margin, scale=None, weights_rank3=True):
    from soft_contrastive_learning_amd.model import losses as M
    zt = torch.tensor(z, device=dev)
    a = zt[:, :1].clone().requires_grad_(True)
    pos = zt[:, 1:1 + p].clone().requires_grad_(True)
    neg = zt[:, 1 + p:].clone().requires_grad_(True)
    if kind == 'neg_eigenvalue':
        loss, terms = M.neg_eigenvalue_loss(a, neg, return_terms=True)
    elif kind in ED.HINGE:
        loss, terms = getattr(M, kind + '_loss')(a, pos, neg, margin, return_terms=True)
    elif kind == 'swrd':
        pwt, nwt = torch.tensor(pw, device=dev), torch.tensor(nw, device=dev)
        if weights_rank3:
            pwt, nwt = pwt[:, :, None], nwt[:, :, None]
        loss, terms = M.swrd_loss(a, pos, neg, pwt, nwt, margin, dimensions=k, return_terms=True)
    else:
        loss, terms = getattr(M, kind + '_loss')(a, pos, neg, margin, dimensions=k, return_terms=True)
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    grads = [np.zeros(x.shape, np.float32) if x.grad is None else x.grad.cpu().numpy() for x in (a, pos, neg)]
    return loss.detach().cpu(), terms.cpu().numpy(), grads


def run_case(kind, shape, dev, c, **kw):
    return run(kind, c['z'], c['pw'], c['nw'], shape[1], shape[4], dev, c['margin'], **kw)


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize('kind', ED.KINDS)
def test_terms_loss_and_gradients_match_the_float64_oracle(dev, kind, shape):
    t, p, n, e, k = shape
    c = oracle(kind, shape)
    loss, terms, (ga, gp, gn) = run_case(kind, shape, dev, c)
    want_grad = c['grad']
    assert terms.dtype == np.float64 and terms.shape == (t, 2)
    err = np.abs(terms - c['terms'])
    g_rel = [_rel(ga, want_grad[:, :1]), _rel(gn, want_grad[:, 1 + p:])]
    if kind == 'neg_eigenvalue':
        assert not gp.any() and not want_grad[:, 1:1 + p].any()
    else:
        g_rel.append(_rel(gp, want_grad[:, 1:1 + p]))
    print('%s %s: margin %.9g, terms err/|term| %.2e, loss %.9g (want %.9g), grads rel %s'
          % (kind, shape, c['margin'], (err / np.maximum(np.abs(c['terms']), 1e-300)).max(), float(loss),
             c['loss'], ['%.2e' % g for g in g_rel]))
    assert (err <= REL * np.abs(c['terms'])).all(), (terms, c['terms'])
    assert abs(float(loss) - c['loss']) <= REL * abs(c['loss']) + 1e-8, (float(loss), c['loss'])
    assert np.abs(want_grad).max() > 0 and max(g_rel) < GRAD_REL, g_rel


@pytest.mark.parametrize('kind', ED.HINGE)
def test_inactive_hinge_gives_zero_loss_and_zero_gradients(dev, kind):
    shape = SHAPES[5]                                     # T = 1
    c = oracle(kind, shape, active=False)
    assert c['loss'] == 0.0 and not c['grad'].any()
    loss, terms, grads = run_case(kind, shape, dev, c)
    assert float(loss) == 0.0
    assert (np.abs(terms - c['terms']) <= REL * np.abs(c['terms'])).all()
    for g in grads:
        assert not g.any()


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize('kind', ['residual_det', 'swrd'])
def test_side_sized_matrix_agrees_with_wrd_on_padded_weights(dev, kind, shape):
    from soft_contrastive_learning_amd.model import losses as M
    t, p, n, e, k = shape
    z, pw, nw = inputs(kind, shape)
    if kind == 'residual_det':                            # indicator weights
        pw, nw = np.ones_like(pw), np.ones_like(nw)
    pad_p = np.concatenate([pw, np.zeros((t, n), np.float32)], 1)
    pad_n = np.concatenate([np.zeros((t, p), np.float32), nw], 1)
    zt = torch.tensor(z, device=dev)
    a, pos, neg = zt[:, :1], zt[:, 1:1 + p], zt[:, 1 + p:]
    _, want = M.wrd_loss(a, pos, neg, torch.tensor(pad_p, device=dev), torch.tensor(pad_n, device=dev),
                         MARGIN, dimensions=k, return_products=True)
    _, got, _ = run(kind, z, pw, nw, p, k, dev, MARGIN)
    rel = np.abs(got - want.cpu().numpy()) / np.abs(want.cpu().numpy())
    print('%s %s: products against wrd rel %.2e' % (kind, shape, rel.max()))
    assert rel.max() <= CROSS_REL, (got, want)


@pytest.mark.parametrize('kind', ED.KINDS)
def test_two_calls_are_bit_identical_and_the_weights_may_be_rank_2(dev, kind):
    shape = SHAPES[3]
    c = oracle(kind, shape)
    one = run_case(kind, shape, dev, c)
    two = run_case(kind, shape, dev, c, weights_rank3=False)
    assert one[0].numpy().tobytes() == two[0].numpy().tobytes()
    assert one[1].tobytes() == two[1].tobytes()
    for a, b in zip(one[2], two[2]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('kind', ED.KINDS)
def test_grad_loss_scales_the_gradient(dev, kind):
    shape = SHAPES[1]
    c = oracle(kind, shape)
    one = run_case(kind, shape, dev, c)
    three = run_case(kind, shape, dev, c, scale=3.0)
    assert max(np.abs(g).max() for g in one[2]) > 0     # (ntuplet_trace: the anchor's own two terms cancel)
    for a, b in zip(one[2], three[2]):
        np.testing.assert_allclose(b, 3.0 * a, rtol=1e-6, atol=0)


def test_golden_losses_and_terms_of_the_reference_are_reproduced(dev, golden_dir):
    from soft_contrastive_learning_amd.model import losses as M
    cases = json.load(open(os.path.join(golden_dir, 'golden_ref_eigen_v1.json')))['losses']
    assert {c['kind'] for c in cases} == set(ED.KINDS) | {'ms_sum'}
    for c in cases:
        t, p, n, k = c['t'], c['p'], c['n'], c['dimensions']
        z, pw, nw = D.tuples(t, p, n, c['e'], c['seed'])
        if c['kind'] == 'ntuplet_trace':
            z = ED.scale_rows(z, c['seed'])
        want = np.asarray(c['terms'])
        if c['kind'] == 'ms_sum':
            zt = torch.tensor(z, device=dev)
            one = np.concatenate((np.zeros(1 + p), np.arange(n) + 1))             # train/train.py:830-834
            labels = np.concatenate([one + b * (n + 1) for b in range(t)])
            loss = M.ms_sum(zt[:, :1], zt[:, 1:1 + p], zt[:, 1 + p:], c['margin'], torch.tensor(labels, device=dev),
                            zt.reshape(t * (1 + p + n), -1), dimensions=k).cpu()
            _, terms, _ = run('residual_det', z, None, None, p, k, dev, c['margin'])
        else:
            loss, terms, _ = run(c['kind'], z, pw[:, :p].copy(), nw[:, p:].copy(), p, k, dev, c['margin'])
        assert (np.abs(terms - want) <= REL * np.abs(want)).all(), (c['kind'], terms, want)
        assert abs(float(loss) - c['loss']) <= REL * abs(c['loss']) + 1e-8, (c['kind'], float(loss), c['loss'])


def test_bad_shapes_raise_before_any_launch(dev):
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.model import losses as M

    def rows(p, n, e=16, t=2):
        return tuple(torch.zeros((t, r, e), device=dev) for r in (1, p, n))

    def ones(*shape):
        return torch.ones(shape, device=dev)

    with _lib.KernelTimer() as timer:
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
                fn(a, pos, neg[:, :, :8], 0.1)                         # another E
            with pytest.raises(ValueError):
                fn(a, pos[:1], neg, 0.1)                               # another T
            with pytest.raises(ValueError):
                fn(a[:, 0], pos, neg, 0.1)                             # rank 2
        a, pos, neg = rows(4, 5)
        for pw, nw in ((ones(2, 5, 1), ones(2, 5, 1)), (ones(2, 4, 1), ones(2, 4, 1)), (ones(2, 4, 2), ones(2, 5, 1)),
                       (ones(2, 9, 1), ones(2, 9, 1)), (None, None)):
            with pytest.raises(ValueError):
                M.swrd_loss(a, pos, neg, pw, nw, 0.1, dimensions=3)
        with pytest.raises(ValueError):
            M.swrd_loss(a, pos, neg, ones(2, 4, 1), ones(2, 5, 1), 0.1, dimensions=5)
        with pytest.raises(ValueError):
            M.neg_eigenvalue_loss(a, torch.zeros((2, 32, 16), device=dev))   # 33 rows with the anchor
        with pytest.raises(ValueError):
            M.neg_eigenvalue_loss(a, neg[:, :0])
    assert timer.records == []


def _train(tmp_path, monkeypatch, loss, extra):
    from soft_contrastive_learning_amd.model import nets
    from soft_contrastive_learning_amd.train import train as T
    before = []
    make = T.make_optimizer

    def spy(kind, params, *a, **k):
        before.extend((q, q.detach().clone()) for q in params)
        return make(kind, params, *a, **k)
    monkeypatch.setattr(T, 'make_optimizer', spy)
    T.main(['--loss', loss, '--steps', '3', '--height', '64', '--width', '80',
            '--positives_per_tuple', '12', '--negatives_per_tuple', '12', '--max_epoch', '1',
            '--tensorboard', '0', '--out_root', str(tmp_path)] + extra)
    recs = [json.loads(l) for l in open(os.path.join(str(tmp_path), loss, 'train_log.txt'))]
    steps = [r['loss'] for r in recs if 'loss' in r and 'event' not in r]
    assert len(steps) == 3 and np.all(np.isfinite(steps)), steps
    assert before and any(not torch.equal(q.detach(), q0) for q, q0 in before)
    nets.set_default_model(None)
    return steps


# lambda_max(neg) <= N + 1 = 13 on unit rows: a margin of 20 keeps the hinge active whatever the weights
@pytest.mark.parametrize('loss,extra', [('residual_trace', []), ('ms_sum', []),
                                        ('ntuplet_evmm', ['--margin_1', '20'])])
def test_trainer_runs_three_steps(dev, tmp_path, monkeypatch, loss, extra):
    steps = _train(tmp_path, monkeypatch, loss, extra)
    if loss == 'ntuplet_evmm':
        assert min(steps) > 0                              # the hinge was active


def test_trainer_runs_ms_sum_under_a_process_group(tmp_path):
    """`--force_dist 1`: a one-rank RCCL group takes compute_loss through its data-parallel branch,
    5 ms_loss_dp on the gathered batch + tuple_loss_dp(residual_det_loss of the local tuples).  A
    process of its own, as tests/test_gpu_rccl.py starts one: the group lives and dies with it."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'SCL_TRAIN_ONE_GPU_GLOO'):
        env.pop(k, None)
    r = subprocess.run(
        [sys.executable, '-m', 'soft_contrastive_learning_amd.train.train', '--loss', 'ms_sum', '--steps', '3',
         '--height', '64', '--width', '80', '--positives_per_tuple', '12', '--negatives_per_tuple', '12',
         '--tuples_per_batch', '2', '--max_epoch', '1', '--force_dist', '1', '--tensorboard', '0',
         '--out_root', str(tmp_path)],
        env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    recs = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'ms_sum', 'train_log.txt'))]
    steps = [x['loss'] for x in recs if 'loss' in x and 'event' not in x]
    assert len(steps) == 3 and np.all(np.isfinite(steps)), steps

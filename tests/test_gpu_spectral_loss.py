"""GPU parity of wrd_loss / prodwrd_loss / sumwrd_loss (csrc/spectral_loss.hip) against a literal
float64 restatement of the reference (model/losses.py:373-437) on torch-CPU ``svdvals`` autograd.

Gates (the project's own, tests/test_gpu_losses.py): every product of ``prods_out`` within 1e-4
relative, the loss within 1e-4 relative + 1e-8, the gradients of anchor, positives and negatives
within GRAD_REL = 2e-4 norm-relative.  The loss alone checks nothing — it is the margin plus a
difference of products of 1e-5 and smaller — so the products are compared one by one.

Inputs: tests/spectral_data.py.  ``dimensions <= min(P, N) - 1`` throughout (with fewer
well-weighted rows than singular values the k-th one is noise in any arithmetic), and every case
asserts on its oracle that s_k / s_1 >= 0.05 and s_k - s_{k+1} >= 1e-6 s_1.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import spectral_data as D

pytestmark = pytest.mark.gpu

REL = 1e-4
GRAD_REL = 2e-4
MARGIN = 0.1
KINDS = ('wrd', 'prodwrd', 'sumwrd')
# (T, P, N, E, dimensions)
SHAPES = [(2, 4, 4, 64, 3),
          (3, 5, 7, 200, 4),            # odd S, E not a multiple of 64
          (2, 12, 12, 512, 10),         # two E slices
          (1, 12, 12, 32768, 10),       # the trainer's shape
          (2, 31, 1, 96, 1)]            # the S = 32 cap


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def reference_f64(kind, z, pos_w, neg_w, p, margin, k, f_alpha_p=2.0, f_alpha_n=50.0, f_lamb=1.0):
    """model/losses.py:373-437 restated on torch float64.  -> loss, prods [T,2], d loss / d z,
    singular values of both sides [2,T,min(S,E)]."""
    z = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    pw = torch.tensor(np.asarray(pos_w, dtype=np.float64))[:, :, None]
    nw = torch.tensor(np.asarray(neg_w, dtype=np.float64))[:, :, None]
    anchor, others = z[:, :1], z[:, 1:]
    residuals = others - anchor
    if kind == 'wrd':
        yp, yn = residuals * pw, residuals * nw
    else:
        sim = anchor @ others.transpose(1, 2)
        fp = (1.0 / (1.0 + torch.exp(f_alpha_p * (sim - f_lamb)))).transpose(1, 2)
        fn = (1.0 / (1.0 + torch.exp(f_alpha_n * (f_lamb - sim)))).transpose(1, 2)
        if kind == 'prodwrd':
            yp, yn = residuals * pw * fp, residuals * nw * fn
        else:
            yp, yn = residuals * (pw + fp), residuals * (nw + fn)
    sp, sn = torch.linalg.svdvals(yp), torch.linalg.svdvals(yn)
    prod_p, prod_n = sp[:, :k].prod(1), sn[:, :k].prod(1)
    loss = (prod_p - prod_n + margin).mean(0)
    loss.backward()
    return (float(loss.detach()), torch.stack([prod_p, prod_n], 1).detach().numpy(), z.grad.numpy(),
            torch.stack([sp, sn]).detach().numpy())


def assert_well_posed(sv, k):
    """The oracle's own singular values: the k-th is not noise and is separated from the next."""
    s1, sk = sv[..., 0], sv[..., k - 1]
    assert (sk / s1).min() >= 0.05, (sk / s1).min()
    if sv.shape[-1] > k:
        assert ((sk - sv[..., k]) / s1).min() >= 1e-6, ((sk - sv[..., k]) / s1).min()


_ORACLE = {}


def oracle(kind, shape, seed=5):
    key = (kind, shape, seed)
    if key not in _ORACLE:
        t, p, n, e, k = shape
        z, pw, nw = D.tuples(t, p, n, e, seed)
        loss, prods, grad, sv = reference_f64(kind, z, pw, nw, p, MARGIN, k)
        assert_well_posed(sv, k)
        for a in (z, pw, nw, prods, grad):
            a.setflags(write=False)
        _ORACLE[key] = (z, pw, nw, loss, prods, grad)
    return _ORACLE[key]


def run(kind, z, pw, nw, p, k, dev, weights_rank3=True, scale=None, margin=MARGIN):
    from soft_contrastive_learning_amd.model import losses as M
    zt = torch.tensor(z, device=dev)
    a = zt[:, :1].clone().requires_grad_(True)
    pos = zt[:, 1:1 + p].clone().requires_grad_(True)
    neg = zt[:, 1 + p:].clone().requires_grad_(True)
    pwt, nwt = torch.tensor(pw, device=dev), torch.tensor(nw, device=dev)
    if weights_rank3:
        pwt, nwt = pwt[:, :, None], nwt[:, :, None]
    loss, prods = getattr(M, kind + '_loss')(a, pos, neg, pwt, nwt, margin, dimensions=k,
                                             return_products=True)
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), prods.cpu().numpy(), [x.grad.cpu().numpy() for x in (a, pos, neg)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'T%d_P%d_N%d_E%d_k%d' % s)
@pytest.mark.parametrize('kind', KINDS)
def test_products_loss_and_gradients_match_the_float64_svd(dev, kind, shape):
    t, p, n, e, k = shape
    z, pw, nw, want_loss, want_prods, want_grad = oracle(kind, shape)
    loss, prods, (ga, gp, gn) = run(kind, z, pw, nw, p, k, dev)
    assert prods.dtype == np.float64 and prods.shape == (t, 2)
    rel = np.abs(prods - want_prods) / np.abs(want_prods)
    g_rel = [_rel(ga, want_grad[:, :1]), _rel(gp, want_grad[:, 1:1 + p]), _rel(gn, want_grad[:, 1 + p:])]
    print('%s %s: products rel %.2e, loss %.9g (want %.9g), grads rel %s'
          % (kind, shape, rel.max(), float(loss), want_loss, ['%.2e' % g for g in g_rel]))
    assert rel.max() <= REL, (prods, want_prods)
    assert abs(float(loss) - want_loss) <= REL * abs(want_loss) + 1e-8, (float(loss), want_loss)
    assert max(g_rel) < GRAD_REL, g_rel


@pytest.mark.parametrize('kind', KINDS)
def test_two_calls_are_bit_identical_and_the_weights_may_be_rank_2(dev, kind):
    shape = SHAPES[2]
    z, pw, nw = oracle(kind, shape)[:3]
    one = run(kind, z, pw, nw, shape[1], shape[4], dev)
    two = run(kind, z, pw, nw, shape[1], shape[4], dev, weights_rank3=False)
    assert one[0].numpy().tobytes() == two[0].numpy().tobytes()
    assert one[1].tobytes() == two[1].tobytes()
    for a, b in zip(one[2], two[2]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('kind', KINDS)
def test_grad_loss_scales_the_gradient(dev, kind):
    shape = SHAPES[1]
    z, pw, nw = oracle(kind, shape)[:3]
    one = run(kind, z, pw, nw, shape[1], shape[4], dev)
    three = run(kind, z, pw, nw, shape[1], shape[4], dev, scale=3.0)
    for a, b in zip(one[2], three[2]):
        assert np.abs(a).max() > 0
        np.testing.assert_allclose(b, 3.0 * a, rtol=1e-6, atol=0)


def test_golden_losses_and_products_of_the_reference_are_reproduced(dev, golden_dir):
    cases = json.load(open(os.path.join(golden_dir, 'golden_ref_wrd_v1.json')))['losses']
    assert {c['kind'] for c in cases} == set(KINDS)
    for c in cases:
        z, pw, nw = D.tuples(c['t'], c['p'], c['n'], c['e'], c['seed'])
        loss, prods, _ = run(c['kind'], z, pw, nw, c['p'], c['dimensions'], dev, margin=c['margin'])
        want = np.asarray(c['prods'])
        assert (np.abs(prods - want) / np.abs(want)).max() <= REL, (c['kind'], prods, want)
        assert abs(float(loss) - c['loss']) <= REL * abs(c['loss']) + 1e-8, (c['kind'], float(loss), c['loss'])


def test_bad_shapes_raise_before_any_launch(dev):
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.model import losses as M

    def call(p, n, k, wshape=None, e=16, fn=M.wrd_loss):
        s = p + n
        a, pos, neg = (torch.zeros((2, r, e), device=dev) for r in (1, p, n))
        w = torch.ones(wshape or (2, s, 1), device=dev)
        return fn(a, pos, neg, w, w, 0.1, dimensions=k)

    with _lib.KernelTimer() as timer:
        for fn in (M.wrd_loss, M.prodwrd_loss, M.sumwrd_loss):
            with pytest.raises(ValueError):
                call(20, 13, 10, fn=fn)                   # S = 33
            with pytest.raises(ValueError):
                call(4, 4, 0, fn=fn)                      # dimensions = 0
            with pytest.raises(ValueError):
                call(4, 4, 9, fn=fn)                      # dimensions = S + 1
            with pytest.raises(ValueError):
                call(4, 4, 3, wshape=(2, 7, 1), fn=fn)    # weights of another S
            with pytest.raises(ValueError):
                call(4, 4, 3, wshape=(2, 8, 2), fn=fn)
    assert timer.records == []


def test_c_abi_validates_on_the_host(dev):
    from soft_contrastive_learning_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    nb = lib.scl_spectral_loss_workspace_bytes(1, 8, 16)
    assert nb > 0 and nb % 256 == 0 and nb <= buf.numel()
    ok = (0, p, p, p, 1, 8, 16, 0.1, 3, 2.0, 50.0, 1.0, p, p, None, p, nb, None)

    def with_(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.scl_spectral_loss_fwd(*a)

    for i in (1, 2, 3, 12, 13, 15):                       # z, weights, loss, products, workspace
        assert with_(**{'a%d' % i: None}) == -3
    assert with_(a5=33) == -1 and with_(a5=0) == -1        # S
    assert with_(a8=0) == -1 and with_(a8=9) == -1         # dimensions
    assert with_(a6=0) == -1 and with_(a4=0) == -1         # E, T
    assert with_(a0=3) == -2 and with_(a0=-1) == -2        # kind
    assert with_(a16=nb - 1) == -4
    assert lib.scl_spectral_loss_workspace_bytes(1, 33, 16) == 0


def _train(tmp_path, monkeypatch, extra):
    from soft_contrastive_learning_amd.model import nets
    from soft_contrastive_learning_amd.train import train as T
    before = []
    make = T.make_optimizer

    def spy(kind, params, *a, **k):
        before.extend((q, q.detach().clone()) for q in params)
        return make(kind, params, *a, **k)
    monkeypatch.setattr(T, 'make_optimizer', spy)
    T.main(['--loss', 'wrd', '--steps', '3', '--height', '64', '--width', '80',
            '--positives_per_tuple', '12', '--negatives_per_tuple', '12', '--max_epoch', '1',
            '--tensorboard', '0', '--out_root', str(tmp_path)] + extra)
    recs = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'wrd', 'train_log.txt'))]
    steps = [r['loss'] for r in recs if 'loss' in r and 'event' not in r]
    assert 1 <= len(steps) <= 3 and np.all(np.isfinite(steps)), steps
    assert before and any(not torch.equal(q.detach(), q0) for q, q0 in before)
    nets.set_default_model(None)
    return steps


def test_trainer_runs_with_the_wrd_loss(dev, tmp_path, monkeypatch):
    assert len(_train(tmp_path, monkeypatch, [])) == 3


def test_trainer_runs_with_the_wrd_loss_on_the_dataset_route(dev, tmp_path, monkeypatch):
    _train(tmp_path, monkeypatch, ['--synthetic_dataset', '400', '--mining_cache_size', '40',
                                   '--num_eval_queries', '8', '--eval_ref_r', '4'])

"""GPU checks of the dense reduction heads (--reduction 1fc|2fc|3fc, csrc/dense.hip): the three
kernels against float64 on ragged and real shapes, their bitwise reproducibility and row
independence, the whole model against the CPU composition, the trainer (one process and the
data-parallel route) and the inference script."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REAL = [(32768, 4096), (84480, 4096), (4096, 4096), (4096, 512), (32768, 512)]
TAILS = [(1000, 100), (4097, 513)]
ROWS = [1, 7, 25, 48, 192, 256]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _within(got, want, bound, what):
    err = (got.double() - want).abs()
    lim = 1e-5 * bound + 1e-30
    worst = float((err / lim).max())
    assert worst <= 1.0, (what, worst, float(err.max()))


def _check_shape(dev, K, N, rows):
    from soft_contrastive_learning_amd.model import reduction as R
    g = torch.Generator(device=dev).manual_seed(K * 7 + N)
    w = torch.randn(K, N, device=dev, generator=g)
    b = torch.randn(N, device=dev, generator=g)
    w64, aw = w.double(), w.double().abs()
    for M in rows:
        relu = M % 2 == 1
        x = torch.randn(M, K, device=dev, generator=g)
        gy = torch.randn(M, N, device=dev, generator=g)
        x64, ax = x.double(), x.double().abs()
        # forward: |err| <= 1e-5 sum_k |x_mk| |w_kn| (+ |b_n|)
        y = R.dense_fwd(x, w, b, relu)
        pre = x64 @ w64 + b.double()
        _within(y, pre.clamp_min(0) if relu else pre, ax @ aw + b.double().abs(), ('fwd', M, K, N))
        # backward-data / weight and bias gradient with g' = gy masked by the saved output
        ys = y if relu else None
        g64 = gy.double() * (y.double() > 0) if relu else gy.double()
        gx = R.dense_bwd_data(gy, ys, w)
        _within(gx, g64 @ w64.t(), g64.abs() @ aw.t(), ('bwd_data', M, K, N))
        gw = torch.empty_like(w)
        gb = torch.empty_like(b)
        R.dense_wgrad(x, gy, ys, gw, gb)
        _within(gw, x64.t() @ g64, ax.t() @ g64.abs(), ('wgrad', M, K, N))
        _within(gb, g64.sum(0), g64.abs().sum(0), ('bgrad', M, K, N))
    torch.cuda.synchronize()


@pytest.mark.parametrize("K,N", TAILS + REAL)
def test_kernels_against_float64(dev, K, N):
    rows = ROWS if (K, N) in TAILS or K * N <= 4096 * 4096 else [1, 25, 192]
    _check_shape(dev, K, N, rows)


def test_unaligned_strides_take_the_scalar_path(dev):
    """Row strides that are not a multiple of 4 floats (views into wider buffers)."""
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.model import reduction as R
    M, K, N = 9, 301, 70
    xb = torch.randn(M, K + 3, device=dev)
    wb = torch.randn(K, N + 1, device=dev)
    x, w = xb[:, 1:K + 1], wb[:, :N]
    b = torch.randn(N, device=dev)
    lib = _lib.load()
    y = torch.empty(M, N + 5, device=dev)
    ws = _lib.workspace(lib.scl_dense_fwd_workspace_bytes(M, K, N), dev)
    _lib.check(lib.scl_dense_fwd(_lib.ptr(x), x.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(b), M, K, N,
                                 0, _lib.ptr(y), y.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_of(x)))
    want = x.double() @ w.double() + b.double()
    _within(y[:, :N], want, x.double().abs() @ w.double().abs() + b.double().abs(), 'fwd strided')
    gy = torch.randn(M, N, device=dev)
    gw = torch.empty(K, N, device=dev)
    R.dense_wgrad(x, gy, None, gw, None)
    _within(gw, x.double().t() @ gy.double(), x.double().abs().t() @ gy.double().abs(), 'wgrad strided')


def test_repeatable_and_rows_independent_of_the_batch(dev):
    """Two calls give the same bits; row m of an M = 25 call equals the M = 1 call on that row
    (the split depends on (K, N) only: the reference's padded inference passes change nothing)."""
    from soft_contrastive_learning_amd.model import reduction as R
    for K, N in [(32768, 512), (4097, 513), (4096, 4096)]:
        g = torch.Generator(device=dev).manual_seed(3)
        w = torch.randn(K, N, device=dev, generator=g)
        b = torch.randn(N, device=dev, generator=g)
        x = torch.randn(25, K, device=dev, generator=g)
        gy = torch.randn(25, N, device=dev, generator=g)
        y1, y2 = R.dense_fwd(x, w, b, True), R.dense_fwd(x, w, b, True)
        assert torch.equal(y1, y2)
        gx1, gx2 = R.dense_bwd_data(gy, y1, w), R.dense_bwd_data(gy, y1, w)
        assert torch.equal(gx1, gx2)
        gws = [torch.empty_like(w) for _ in range(2)]
        gbs = [torch.empty_like(b) for _ in range(2)]
        for gw, gb in zip(gws, gbs):
            R.dense_wgrad(x, gy, y1, gw, gb)
        assert torch.equal(gws[0], gws[1]) and torch.equal(gbs[0], gbs[1])
        for m in (0, 13, 24):
            assert torch.equal(R.dense_fwd(x[m:m + 1], w, b, True)[0], y1[m])
            assert torch.equal(R.dense_bwd_data(gy[m:m + 1], y1[m:m + 1], w)[0], gx1[m])


def test_two_forward_passes_in_training_mode_are_bit_equal(dev):
    """No dropout (tf.layers.dropout with training=False, model/reduction.py)."""
    from soft_contrastive_learning_amd.model import reduction as R
    head = R.DenseHead('3fc', 512, 64).to(dev).train()
    x = torch.randn(25, 512, device=dev)
    assert torch.equal(head(x), head(x))


@pytest.mark.parametrize("vlad_cores,hw,kind", [(64, (64, 80), '1fc'), (64, (64, 80), '3fc'),
                                                 (0, (180, 240), '1fc'), (0, (180, 240), '3fc')])
def test_whole_model_against_the_cpu_composition(dev, vlad_cores, hw, kind):
    """Forward and parameter gradients of backbone + head on the GPU against the CPU composition:
    the whole CPU model without NetVLAD; with it (whose kernels exist on the GPU only) the CPU head on
    the GPU's descriptors, and the gradient reaching the descriptors."""
    from soft_contrastive_learning_amd.model import nets, reduction
    h, w = hw
    gpu = nets.VGG16NetVLAD(vlad_cores=vlad_cores, seed=5).to(dev)
    reduction.attach(gpu, kind, 128, height=h, width=w, seed=6)
    img = torch.rand(3, h, w, 3, generator=torch.Generator().manual_seed(1)) * 255
    coef = torch.randn(3, 128, generator=torch.Generator().manual_seed(2))
    full = nets.full_out(img.to(dev), model=gpu)
    full.retain_grad()
    out = gpu.reduction_head(full)
    (out * coef.to(dev)).sum().backward()
    if vlad_cores == 0:
        cpu = nets.VGG16NetVLAD(vlad_cores=0, seed=5)
        reduction.attach(cpu, kind, 128, height=h, width=w, seed=6)
        out_c = nets.output(img, model=cpu)
        params = [(n, p, dict(cpu.named_parameters())[n]) for n, p in gpu.named_parameters()]
    else:
        head = reduction.DenseHead(kind, 32768, 128, seed=6)
        full_c = full.detach().cpu().requires_grad_(True)
        out_c = head(full_c)
        params = [(n, p, dict(head.named_parameters())[n[len('reduction_head.'):]])
                  for n, p in gpu.named_parameters() if n.startswith('reduction_head.')]
    (out_c * coef).sum().backward()
    assert out.shape == (3, 128)
    o_c = out_c.detach().numpy()
    np.testing.assert_allclose(out.detach().cpu().numpy(), o_c, rtol=2e-3, atol=2e-5 * np.abs(o_c).max())
    if vlad_cores:
        ref = full_c.grad
        assert float((full.grad.cpu() - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    for n, pg, pc in params:
        if pc.grad is None:
            assert pg.grad is None, n
            continue
        ref = pc.grad
        err = float((pg.grad.cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        # the backbone's convolutions run bf16 operands on the matrix cores (tests/test_gpu_backbone.py
        # gates them at 5e-2); the float32 head at 2e-3
        assert err <= (2e-3 if n.startswith('reduction_head') else 5e-2), (n, err)


def test_trainer_3fc_writes_and_trains_the_head(dev, tmp_path):
    from soft_contrastive_learning_amd import checkpoint
    from soft_contrastive_learning_amd.model import nets, reduction
    from soft_contrastive_learning_amd.train import train as T
    T.main(['--loss', 'triplet', '--reduction', '3fc', '--out_dim', '256', '--height', '64', '--width', '80',
            '--positives_per_tuple', '2', '--negatives_per_tuple', '2', '--margin_1', '0.5',
            '--steps', '3', '--max_epoch', '1', '--base_lr', '1e-4', '--out_root', str(tmp_path)])
    model = nets.default_model()
    head = reduction.head_of(model)
    assert head is not None and head.in_dim == 32768 and head.out_dim == 256
    recs = [l for l in open(os.path.join(str(tmp_path), 'triplet', 'train_log.txt'))]
    import json
    losses = [json.loads(l)['loss'] for l in recs]
    assert len(losses) == 3 and np.all(np.isfinite(losses))
    # the gradients reached the head through the buckets (.grad is a view of the flat buffer)
    # (the last bias cancels out of every distance: its gradient is zero)
    for name, p in head.tf_variables():
        assert p.grad is not None and (name == 'fc3/bias' or float(p.grad.abs().sum()) > 0), name
    fresh = reduction.DenseHead('3fc', 32768, 256)
    assert not torch.equal(head.dense_kernel.detach().cpu(), fresh.dense_kernel)
    ck = [f for f in (tmp_path / 'triplet').iterdir() if f.name.endswith('.index')]
    sd = checkpoint.read_variables(str(sorted(ck)[0]))
    for name in ('dense/kernel', 'dense_1/kernel', 'fc3/kernel', 'fc3/bias', 'dense/kernel/Adam'):
        assert name in sd, name
    assert sd['dense/kernel'].shape == (32768, 4096) and sd['fc3/kernel'].shape == (4096, 256)
    nets.set_default_model(None)


def _dist_worker(rank, port, out):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port), SCL_TRAIN_ONE_GPU_GLOO='1')
    from soft_contrastive_learning_amd.model import nets, reduction
    from soft_contrastive_learning_amd.train import train as T
    T.main(['--loss', 'wms', '--reduction', '2fc', '--out_dim', '128', '--height', '64', '--width', '80',
            '--positives_per_tuple', '2', '--negatives_per_tuple', '2', '--steps', '2', '--max_epoch', '1',
            '--base_lr', '1e-4', '--tensorboard', '0', '--out_root', os.path.join(out, 'r%d' % rank)])
    head = reduction.head_of(nets.default_model())
    torch.save({k: p.detach().cpu() for k, p in head.tf_variables()}, os.path.join(out, 'head%d.pt' % rank))


def test_data_parallel_2fc_keeps_the_ranks_equal(tmp_path):
    """Two ranks on one GPU (gloo): the out_dim-wide rows are all-gathered for the wms loss and the
    head gradients are summed by the buckets — both ranks end with the same head."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_dist_worker, args=(r, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    a, b = (torch.load(os.path.join(str(tmp_path), 'head%d.pt' % r)) for r in range(2))
    from soft_contrastive_learning_amd.model import reduction
    init = dict(reduction.DenseHead('2fc', 32768, 128).tf_variables())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['dense/kernel'], init['dense/kernel'].detach())


def test_inference_writes_out_dim_wide_descriptors(dev, tmp_path):
    from soft_contrastive_learning_amd.evaluation import inference
    inference.main(['--reduction', '1fc', '--out_dim', '256', '--num_images', '3', '--small_side', '64',
                    '--large_side', '80', '--images_per_pass', '2', '--out_root', str(tmp_path)])
    with open(os.path.join(str(tmp_path), 'synthetic_scl_amd.pickle'), 'rb') as f:
        feats = pickle.load(f)
    assert len(feats) == 3 and all(f.shape == (256,) and f.dtype == np.float32 for f in feats)
    assert all(np.isfinite(f).all() for f in feats)

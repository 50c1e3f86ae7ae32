"""The exact references of tests/exact_conv.py against torch's float64 CPU operators, so that the
GPU tests built on them (tests/test_gpu_conv_exact.py) rest on a helper checked independently of
any kernel: odd and even maps, maps of height or width 2, tie-heavy pooling windows."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_conv as X

CPU = torch.device('cpu')
SHAPES = [(2, 7, 9), (1, 8, 10), (2, 2, 6), (1, 5, 2), (1, 2, 2), (3, 13, 11)]


def _operands(seed, b, cin, kout, h, w):
    g = X.generator(seed, CPU)
    x = X.small_ints((b, cin, h, w), -3, 3, g, CPU, torch.float64)
    wt = X.small_ints((kout, cin, 3, 3), -3, 3, g, CPU, torch.float64)
    return x, wt, g


@pytest.mark.parametrize('b,h,w', SHAPES)
@pytest.mark.parametrize('cin,kout', [(3, 5), (8, 4)])
def test_forward_and_backward_data_match_torch(b, h, w, cin, kout):
    x, wt, g = _operands(1 + h * w + cin, b, cin, kout, h, w)
    bias = X.int_bias(kout, g, CPU).double()
    want = F.conv2d(x, wt, bias, padding=1)
    got = X.conv3x3(x, wt, bias)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert torch.equal(X.conv3x3(x, wt, out_dtype=torch.float32), F.conv2d(x, wt, padding=1).float())
    gz = X.small_ints((b, kout, h, w), -3, 3, g, CPU, torch.float64)
    assert torch.equal(X.conv3x3_t(gz, wt), F.conv_transpose2d(gz, wt, padding=1))


@pytest.mark.parametrize('b,h,w', SHAPES)
def test_weight_and_bias_gradient_match_autograd(b, h, w):
    x, wt, g = _operands(7 + h + w, b, 6, 4, h, w)
    wr = wt.clone().requires_grad_(True)
    br = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    gz = X.small_ints((b, 4, h, w), -3, 3, g, CPU, torch.float64)
    F.conv2d(x, wr, br, padding=1).backward(gz)
    assert torch.equal(X.conv3x3_wgrad(x, gz), wr.grad)
    assert torch.equal(X.bias_grad(gz), br.grad)


def test_chunking_over_images_changes_nothing(monkeypatch):
    x, wt, g = _operands(5, 5, 4, 3, 6, 7)
    gz = X.small_ints((5, 3, 6, 7), -3, 3, g, CPU, torch.float64)
    whole = (X.conv3x3(x, wt), X.conv3x3_t(gz, wt), X.conv3x3_wgrad(x, gz), X.bias_grad(gz))
    real = X._chunks
    monkeypatch.setattr(X, '_chunks', lambda b, per, budget=0: real(b, per, budget=per * 2))
    assert X._chunks(5, 10) == [(0, 2), (2, 4), (4, 5)]
    parts = (X.conv3x3(x, wt), X.conv3x3_t(gz, wt), X.conv3x3_wgrad(x, gz), X.bias_grad(gz))
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


@pytest.mark.parametrize('h,w', [(2, 2), (4, 6), (5, 7), (3, 2), (9, 13)])
def test_maxpool_index_is_the_first_maximum_like_max_pool2d(h, w):
    g = X.generator(11 + h * w, CPU)
    # values in {0, 1}: nearly every window has a tie
    z = X.small_ints((2, 16, h, w), 0, 1, g, CPU, torch.float64)
    m, idx = X.maxpool2x2(z)
    want, flat = F.max_pool2d(z, 2, 2, return_indices=True)
    assert torch.equal(m, want)
    # max_pool2d returns the flat index h * W + w of the chosen element
    ho, wo = h // 2, w // 2
    py = torch.arange(ho).view(1, 1, ho, 1)
    px = torch.arange(wo).view(1, 1, 1, wo)
    pos = (flat // w - 2 * py) * 2 + (flat % w - 2 * px)
    assert torch.equal(idx.long(), pos)
    ties = (torch.stack([z[:, :, dy:2 * ho:2, dx:2 * wo:2] for dy in (0, 1) for dx in (0, 1)], -1)
            == m[..., None]).sum(-1) > 1
    assert float(ties.double().mean()) > 0.5
    # every raster position wins somewhere, so a fixed answer would not pass
    assert set(idx.unique().tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize('h,w', [(2, 2), (4, 6), (5, 7), (9, 13)])
def test_unpool_is_the_gradient_of_max_pool2d(h, w):
    g = X.generator(3 + h * w, CPU)
    z = X.small_ints((2, 8, h, w), -1, 1, g, CPU, torch.float64).requires_grad_(True)
    m, idx = X.maxpool2x2(z.detach())
    ga = X.small_ints(tuple(m.shape), -3, 3, g, CPU, torch.float64)
    F.max_pool2d(z, 2, 2).backward(ga)
    got = X.unpool(ga, idx, h, w)
    assert torch.equal(got, z.grad)
    # relu(pool(z) + bias)' routes ga * [a > 0] to the same place
    bias = X.int_bias(8, g, CPU).double()
    a = torch.relu(m + bias[None, :, None, None])
    z.grad = None
    torch.relu(F.max_pool2d(z, 2, 2) + bias[None, :, None, None]).backward(ga)
    assert torch.equal(X.unpool(torch.where(X.relu_mask(a), ga, 0.0), idx, h, w), z.grad)


def test_premise_and_rounding_helpers():
    x = torch.full((1, 4, 3, 3), 2.0, dtype=torch.float64)
    wt = torch.full((2, 4, 3, 3), -3.0, dtype=torch.float64)
    # the centre output sums 36 products of magnitude 6
    assert X.premise(X.conv3x3, x, wt) == 216.0
    assert X.premise(X.conv3x3, x, wt, extra=4) == 220.0
    with pytest.raises(AssertionError):
        X.premise(X.conv3x3, x, wt, limit=216)
    v = torch.tensor([255.0, 256.0, 257.0, 259.0, 261.0, -259.0, 2 ** 20 + 2 ** 12], dtype=torch.float64)
    got = X.to_bf16(v).double()
    # ties to even: 257 -> 256, 259 -> 260, 261 -> 260; 2^20 + 2^12 is halfway -> 2^20
    assert got.tolist() == [255.0, 256.0, 256.0, 260.0, 260.0, -260.0, 2.0 ** 20]
    assert X.not_bf16_fraction(v) == pytest.approx(5 / 7)


def test_generators_hit_their_regimes():
    g = X.generator(5, CPU)
    x, wt = X.r1_operands(2, 64, 64, 9, 11, g, CPU)
    assert x.dtype == wt.dtype == torch.bfloat16 and set(x.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert X.premise(X.conv3x3, x, wt, limit=X.BF16_EXACT + 1) <= X.BF16_EXACT
    z = X.conv3x3(x, wt)
    assert float((z == 0).double().mean()) > 0.05
    x, wt = X.r2_operands(1, 512, 4, 6, 7, g, CPU)
    assert X.premise(X.conv3x3, x, wt) < 9 * 512 * 9
    z = X.conv3x3(x, wt)
    assert X.not_bf16_fraction(z) > 0.5
    m = X.halfway_master((64, 64, 3, 3), g, CPU)
    half = m.abs() > 256
    assert 0.15 < float(half.double().mean()) < 0.35
    # every such value lies exactly between two bf16 neighbours: the cast must round
    assert bool((m[half].bfloat16().float() != m[half]).all())
    assert bool((m[half].bfloat16().float() - m[half]).abs().eq(1).all())

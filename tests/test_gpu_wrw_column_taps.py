"""Weight-gradient kernel (csrc/conv_wrw.hip, wrw64_kernel): the column taps as shifted LDS reads.

The kernel reads the x fragment of a window row three times, at pixel offsets 0 / 1 / 2 of the halo
window, one read per column tap, against the unshifted gradient fragment of the step.  What can go
wrong is a halo or an offset: a window column of the neighbouring tile that is missing, doubled or
not zero outside the image, in any of the three staging modes or next to a tile built from a pooled
gradient, a tap that reads the wrong offset, and pixels counted twice into the bias gradient.
Everything goes through ``nets.wrw64``.

Reference: weight and bias gradient on the CPU in float64 from the same bf16 operands (unfold +
einsum).  x and gz are integers in [-4, 4]: every product is an integer of at most 16, every sum
over at most 1,200 pixels stays below 2^15 — far below 2^24, where float32 accumulates exactly in
any order — so the comparison is ``torch.equal`` after the cast to the output dtype.

Shapes (B, H, W) are the smallest at which each piece can go wrong.  The launch takes the tile
shape that cuts the map into fewer tiles (8 x 32 / 32 x 8 for 64 output channels, 4 x 32 / 16 x 8
for 128 and more, wide on a tie); ``_tall`` restates that rule.  Of WIDE, (2, 10, 38) runs on tall
tiles at 128 output channels (10 against 12 tiles) and on wide ones at 64; of TALL, (2, 12, 16)
is a tie at 64 output channels and runs wide there.  Both geometries see every shape family.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
WIDE = [(1, 4, 32), (1, 6, 34), (2, 10, 38), (1, 8, 64)]
TALL = [(1, 32, 8), (1, 34, 10), (2, 12, 16), (1, 30, 40)]
CHANNELS = [(64, 64), (64, 128), (128, 128)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tall(shape, kout):
    """The tile shape csrc/conv_wrw.hip's wrw_plan takes."""
    b, h, w = shape
    th_w, th_t = (4, 16) if kout % 128 == 0 else (8, 32)
    return b * -(-h // th_t) * -(-w // 8) < b * -(-h // th_w) * -(-w // 32)


def test_shape_lists_reach_both_tile_shapes():
    for s in WIDE:
        assert not _tall(s, 64) and (s == (2, 10, 38) or not _tall(s, 128))
    for s in TALL:
        assert _tall(s, 128) and (s == (2, 12, 16) or _tall(s, 64))


def _ints(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)


def _reference(x, gz):
    """(dW [K,C,3,3], db [K]) in float64 on the CPU from bf16 operands [B,C,H,W], [B,K,H,W]."""
    xd, gd = x.cpu().double(), gz.cpu().double()
    b, c, h, w = xd.shape
    k = gd.shape[1]
    cols = F.unfold(xd, 3, padding=1).view(b, c, 9, h * w)
    gw = torch.einsum('bkp,bctp->kct', gd.reshape(b, k, h * w), cols).view(k, c, 3, 3)
    return gw, gd.sum(dim=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def _case(cin, kout, shape):
    """Operands (CPU, bf16) and their reference, computed once per (channels, shape)."""
    b, h, w = shape
    x = _ints((b, cin, h, w), 11 + cin + h * w)
    gz = _ints((b, kout, h, w), 13 + kout + h * w)
    gw, gb = _reference(x, gz)
    assert float(gw.abs().max()) < 2 ** 24 and float(gb.abs().max()) < 2 ** 24
    return x, gz, gw, gb


def _same(got, want, what):
    want = want.to(got.dtype)
    got = got.cpu()
    if torch.equal(got, want):
        return
    bad = got != want
    first = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError('%s: %d of %d differ; first at %s: got %r want %r' % (
        what, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


def _same_taps(got, want, what):
    """All nine taps separately: a wrong halo is one wrong tap."""
    for kh in range(3):
        for kw in range(3):
            _same(got[:, :, kh, kw], want[:, :, kh, kw], '%s, tap (kh %d, kw %d)' % (what, kh, kw))


def _run(x, gz, dev, dtype=torch.float32, pool_idx=None):
    from soft_contrastive_learning_amd.model import nets
    kout, cin = gz.shape[1], x.shape[1]
    like = torch.empty(kout, cin, 3, 3, device=dev, dtype=dtype)
    gb = torch.full((kout,), 7.0, device=dev)
    idx = None if pool_idx is None else pool_idx.to(dev).contiguous(memory_format=CL)
    gw = nets.wrw64(x.to(dev).contiguous(memory_format=CL), gz.to(dev).contiguous(memory_format=CL), like, gb,
                    pool_idx=idx)
    torch.cuda.synchronize()
    return gw, gb


def _ids(shapes):
    return ['%dx%dx%d' % s for s in shapes]


@pytest.mark.parametrize('cin,kout', CHANNELS, ids=['%dx%d' % c for c in CHANNELS])
@pytest.mark.parametrize('shape', WIDE + TALL, ids=_ids(WIDE + TALL))
def test_integer_data_is_exact(dev, cin, kout, shape):
    """Weight gradient tap by tap and bias gradient (= the sum of gz: halo pixels not counted)."""
    x, gz, gw, gb = _case(cin, kout, shape)
    got, got_b = _run(x, gz, dev)
    _same_taps(got, gw, 'weight gradient')
    _same(got_b, gb, 'bias gradient')
    got, got_b = _run(x, gz, dev, torch.bfloat16)
    _same(got, gw, 'weight gradient (bf16)')
    _same(got_b, gb, 'bias gradient (bf16 weights)')


@pytest.mark.parametrize('shape', [(2, 10, 38), (1, 30, 40)], ids=_ids([(2, 10, 38), (1, 30, 40)]))
def test_sibling_workgroups_share_tiles(dev, shape):
    """256 x 256 channels: 4 x 2 workgroups walk the same tiles."""
    x, gz, gw, gb = _case(256, 256, shape)
    got, got_b = _run(x, gz, dev)
    _same_taps(got, gw, 'weight gradient')
    _same(got_b, gb, 'bias gradient')


# gz non-zero in ONE image column only, x non-zero everywhere: the taps kw = 0 and kw = 2 of that
# column take their x pixel from the window's halo column (interior tile borders: the neighbouring
# tile's pixels) or meet the zero padding (image columns 0 and W - 1).
IMPULSE = [((1, 8, 64), (0, 63, 31, 32)), ((1, 6, 34), (0, 33, 31, 32)),
           ((1, 30, 40), (0, 39, 7, 8, 31, 32)), ((1, 34, 10), (0, 9, 7, 8))]


@pytest.mark.parametrize('cin,kout', [(64, 64), (64, 128)], ids=['64x64', '64x128'])
@pytest.mark.parametrize('shape,columns', IMPULSE, ids=_ids([s for s, _ in IMPULSE]))
def test_gradient_in_one_column(dev, cin, kout, shape, columns):
    b, h, w = shape
    g = torch.Generator().manual_seed(5 + h * w)
    x = (torch.randint(1, 5, (b, cin, h, w), generator=g)
         * (1 - 2 * torch.randint(0, 2, (b, cin, h, w), generator=g))).to(torch.bfloat16)
    full = _ints((b, kout, h, w), 17 + h * w, 1, 4)
    for col in columns:
        gz = torch.zeros_like(full)
        gz[:, :, :, col] = full[:, :, :, col]
        gw, gb = _reference(x, gz)
        got, got_b = _run(x, gz, dev)
        _same_taps(got, gw, 'gz in column %d only' % col)
        _same(got_b, gb, 'bias gradient, gz in column %d only' % col)


def _unpool(ga, idx, h, w):
    """Full-size gradient [B,K,H,W] of a 2x2 max-pooling from the pooled one and its window index."""
    b, k = ga.shape[:2]
    out = torch.zeros(b, k, h, w, dtype=ga.dtype)
    for pos in range(4):
        out[:, :, pos >> 1::2, pos & 1::2] = torch.where(idx == pos, ga, torch.zeros_like(ga))
    return out


POOLED = [(1, 10, 38), (1, 14, 70), (1, 18, 32), (1, 34, 16)]


@pytest.mark.parametrize('cin,kout', [(64, 64), (128, 128)], ids=['64x64', '128x128'])
@pytest.mark.parametrize('shape', POOLED, ids=_ids(POOLED))
@pytest.mark.parametrize('index', ['random', 'zeros', 'threes'])
def test_pooled_gradient_builds_the_same_tile(dev, cin, kout, shape, index):
    """The tile built in LDS from the pooled gradient against the plain path on the un-pooled
    gradient: random bf16 data, bit-identical."""
    b, h, w = shape
    g = torch.Generator().manual_seed(23 + h * w + cin)
    x = torch.randn((b, cin, h, w), generator=g).to(torch.bfloat16)
    ga = torch.randn((b, kout, h // 2, w // 2), generator=g).to(torch.bfloat16)
    if index == 'random':
        idx = torch.randint(0, 4, ga.shape, generator=g, dtype=torch.uint8)
    else:
        idx = torch.full(ga.shape, 0 if index == 'zeros' else 3, dtype=torch.uint8)
    plain, plain_b = _run(x, _unpool(ga, idx, h, w), dev)
    pooled, pooled_b = _run(x, ga, dev, pool_idx=idx)
    assert float(plain.abs().max()) > 0
    _same_taps(pooled, plain.cpu(), 'pooled against plain')
    _same(pooled_b, plain_b.cpu(), 'bias gradient, pooled against plain')


@pytest.mark.parametrize('shape', [(2, 12, 16), (2, 10, 38)], ids=_ids([(2, 12, 16), (2, 10, 38)]))
def test_staging_with_and_without_the_buffer_path(dev, shape):
    """The product against diagnostic variant 2200 (per-lane border tests in place of the buffer
    resource) on random bf16 data: the same tile either way, bit-identical."""
    from soft_contrastive_learning_amd import _lib
    b, h, w = shape
    g = torch.Generator().manual_seed(31 + h * w)
    x = torch.randn((b, 128, h, w), generator=g).to(torch.bfloat16)
    gz = torch.randn((b, 128, h, w), generator=g).to(torch.bfloat16)
    got, got_b = _run(x, gz, dev)
    with _lib.variant(2200):
        ab, ab_b = _run(x, gz, dev)
    assert float(got.abs().max()) > 0
    _same_taps(ab, got.cpu(), 'variant 2200 against the product')
    _same(ab_b, got_b.cpu(), 'bias gradient, variant 2200 against the product')

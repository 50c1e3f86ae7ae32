"""Weight-gradient kernel (csrc/conv_wrw.hip, wrw64_kernel): the half-tile schedule (SCHED 1).

On [64 c] x [128 k] blocks the kernel can stage HALF tiles into a ring of four LDS slots, with waves
4-7 running one half behind waves 0-3.  Every wave issues the products of the whole-tile schedule in
the same order into the same accumulators, so the results must not differ by a bit: the whole-tile
schedule (diagnostic variant 2400) is the reference, ``torch.equal`` the comparison, on seeded bf16
data (x after a ReLU: it has zeros; gz signed), weight and bias gradient, through ``nets.wrw64``.
The half-tile schedule is run both as the diagnostic variant 2404 (always SCHED 1) and as the
product picks per instantiation (wrw_sched).

What can go wrong is the ring and the offset between the wave halves: a slot overwritten before its
last reader left, read before it landed, a half staged from the wrong place (the halves of a wide
tile are column halves, of a tall one row halves; either may lie outside the image), a barrier
missed by a wave that walks fewer tiles, the pooled gradient built by the wrong wave half.

Shapes, with the plan csrc/conv_wrw.hip's wrw_plan makes of them on 256 compute units (``_plan``
restates it, and the test of the list checks it where the suite runs): every one of the four
instantiations walks at least three tiles per workgroup — each of the four slots is reused — with
workgroups of one launch walking unequal numbers of tiles.

  512 -> 512, 3 x 30 x 40          tall, 30 tiles over 8 splits (4 or 3 each), rows below the map
  256 -> 256, 3 x 60 x 80          tall, 120 tiles over 32 splits (4 or 3)
   64 -> 128, 2 x 224 x 224        wide, 784 tiles over 256 splits (4 or 3)
  128 -> 128, 2 x 224 x 224 pooled wide, 784 tiles over 128 splits (7 or 6)
  512 -> 512, 3 x 60 x 84  pooled  tall, 132 tiles over 8 splits (17 or 16), columns right of the map
  128 -> 128, 3 x 135 x 241        wide, 816 tiles over 128 splits; H and W no multiples of the tile:
                                   staging modes 1 (rows outside) and 2 (columns outside)
  128 -> 128, 3 x 61 x 43          tall, 72 tiles, as many splits: one tile per workgroup
  128 -> 128, 1 x 4 x 32           one tile: one workgroup walks it, its sibling blocks too
"""
import functools

import pytest
import torch

from tests.util_guard import FILL, Guarded

pytestmark = pytest.mark.gpu

CL = torch.channels_last
WHOLE, HALVES = 2400, 2404
# (cin, kout, (B, H, W), pooled, tall, tiles, splits)
CASES = [
    (512, 512, (3, 30, 40), False, True, 30, 8),
    (256, 256, (3, 60, 80), False, True, 120, 32),
    (64, 128, (2, 224, 224), False, False, 784, 256),
    (128, 128, (2, 224, 224), True, False, 784, 128),
    (512, 512, (3, 60, 84), True, True, 132, 8),
    (128, 128, (3, 135, 241), False, False, 816, 128),
    (128, 128, (3, 61, 43), False, True, 72, 72),
    (128, 128, (1, 4, 32), False, False, 1, 1),
]
IDS = ['%dx%d-%dx%dx%d%s' % ((c[0], c[1]) + c[2] + ('-pooled' if c[3] else '',)) for c in CASES]
RING = CASES[:5]            # at least three tiles per workgroup, unequal numbers of them


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _plan(cin, kout, shape, cus):
    """(tall, tiles, splits) of wrw_plan on [64 c] x [128 k] blocks."""
    b, h, w = shape
    wide, tall = b * -(-h // 4) * -(-w // 32), b * -(-h // 16) * -(-w // 8)
    tiles = min(wide, tall)
    blocks = (cin // 64) * (kout // 128)
    return tall < wide, tiles, max(1, min(-(-cus // blocks), tiles, 1024))


def test_shapes_are_planned_as_listed(dev):
    from soft_contrastive_learning_amd import _lib as L
    cus = max(1, torch.cuda.get_device_properties(dev).multi_processor_count - L.load().scl_get_reserve_cus())
    seen = set()
    for cin, kout, shape, pooled, tall, tiles, splits in CASES:
        assert kout % 128 == 0
        assert _plan(cin, kout, shape, 256) == (tall, tiles, splits)
        seen.add((tall, pooled))
    assert len(seen) == 4                                    # the four instantiations with NKB = 2
    for cin, kout, shape, pooled, tall, tiles, splits in RING:
        t, n, p = _plan(cin, kout, shape, cus)               # ... on the device at hand
        assert n >= 3 * p + 1 and n % p != 0, (cin, kout, shape, n, p)


@functools.lru_cache(maxsize=None)
def _operands(i):
    """Seeded operands of CASES[i] on the CPU: x = relu(randn), gz = randn, both bf16 (+ window index)."""
    cin, kout, (b, h, w), pooled = CASES[i][:4]
    g = torch.Generator().manual_seed(101 + i)
    x = torch.relu(torch.randn((b, cin, h, w), generator=g)).to(torch.bfloat16)
    gh, gw_ = (h // 2, w // 2) if pooled else (h, w)
    gz = torch.randn((b, kout, gh, gw_), generator=g).to(torch.bfloat16)
    idx = torch.randint(0, 4, (b, kout, gh, gw_), generator=g, dtype=torch.uint8) if pooled else None
    return x, gz, idx


@functools.lru_cache(maxsize=None)
def _on_device(i, dev):
    x, gz, idx = _operands(i)
    put = lambda t: None if t is None else t.to(dev).contiguous(memory_format=CL)
    return put(x), put(gz), put(idx)


def _run(i, dev, v):
    """(weight gradient, bias gradient) of CASES[i] as bytes; v: 0 the product, else the variant."""
    from soft_contrastive_learning_amd import _lib as L
    from soft_contrastive_learning_amd.model import nets
    x, gz, idx = _on_device(i, dev)
    like = torch.empty(gz.shape[1], x.shape[1], 3, 3, device=dev)
    gb = torch.full((gz.shape[1],), 7.0, device=dev)
    with L.maybe_variant(v):
        gw = nets.wrw64(x, gz, like, gb, pool_idx=idx)
        torch.cuda.synchronize()
    return gw.cpu(), gb.cpu()


@functools.lru_cache(maxsize=None)
def _whole(i, dev):
    """The whole-tile schedule's result, computed once per case and left unchanged."""
    gw, gb = _run(i, dev, WHOLE)
    assert float(gw.abs().max()) > 0 and float(gb.abs().max()) > 0 and bool(torch.isfinite(gw).all())
    return gw, gb


def _same(got, want, what):
    if torch.equal(got, want):
        return
    bad = got != want
    first = tuple(int(j) for j in bad.nonzero()[0])
    raise AssertionError('%s: %d of %d differ; first at %s: got %r want %r' % (
        what, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
@pytest.mark.parametrize('v', [HALVES, 0], ids=['halves', 'product'])
def test_bits_of_the_whole_tile_schedule(dev, i, v):
    want, want_b = _whole(i, dev)
    got, got_b = _run(i, dev, v)
    _same(got, want, 'weight gradient')
    _same(got_b, want_b, 'bias gradient')


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_same_call_twice_gives_equal_bits(dev, i):
    """No half slot is read before it has landed: nothing depends on the timing of a run."""
    a, a_b = _run(i, dev, HALVES)
    b, b_b = _run(i, dev, HALVES)
    _same(b, a, 'weight gradient, second call')
    _same(b_b, a_b, 'bias gradient, second call')


GUARDED = [0, 2, 3, 4]      # one case per instantiation


@pytest.mark.parametrize('i', GUARDED, ids=[IDS[i] for i in GUARDED])
def test_workspace_between_guard_bands(dev, i):
    """Exactly scl_wrw3x3_workspace_bytes between guard bands, full of 0xA5 and zeroed: the bands
    come back untouched and the outputs are equal, bit for bit."""
    from soft_contrastive_learning_amd import _lib as L
    cin, kout, (b, h, w), pooled = CASES[i][:4]
    x, gz, idx = _on_device(i, dev)
    runs = []
    with L.variant(HALVES) as lib:
        nbytes = lib.scl_wrw3x3_workspace_bytes(cin, kout)
        for fill in (FILL, 0):
            ws = Guarded(dev, nbytes, fill)
            gw = torch.full((kout, cin, 3, 3), 7, dtype=torch.bfloat16, device=dev)
            gb = torch.full((kout,), 7, dtype=torch.float32, device=dev)
            if pooled:
                L.check(lib.scl_wrw3x3_pooled(L.ptr(x), L.ptr(gz), L.ptr(idx), b, h, w, cin, kout, L.ptr(gw),
                                              *gw.stride(), 0, L.ptr(gb), L.ptr(ws.inner), nbytes, L.stream_of(x)))
            else:
                L.check(lib.scl_wrw3x3_bias(L.ptr(x), L.ptr(gz), b, h, w, cin, kout, L.ptr(gw), *gw.stride(), 0,
                                            L.ptr(gb), L.ptr(ws.inner), nbytes, L.stream_of(x)))
            ws.assert_bands_intact()
            runs.append((gw.cpu(), gb.cpu()))
            del ws
    _same(runs[1][0].float(), runs[0][0].float(), 'weight gradient, zeroed against filled workspace')
    _same(runs[1][1], runs[0][1], 'bias gradient, zeroed against filled workspace')

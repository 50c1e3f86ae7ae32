"""Bit-exact checks of the own backbone kernels (csrc/conv64.hip, conv_wrw.hip, conv_lds.hip with
convh.hip and convg.hip, conv_pack.hip, vgg_glue.hip) on integer-valued data.

With small-integer bf16 operands every product is exact and, while every partial sum is an integer
below 2^24 (``exact_conv.premise``, asserted first in every test), the float32 accumulation is
exact in any order: each kernel result must equal the float64 reference of tests/exact_conv.py bit
for bit — bf16 outputs rounded once, to nearest even — and so must the discrete decisions, the
ReLU mask and the max-pool window index (first maximum in raster order) under ties.  No
tolerances.  Two data regimes: R1 (sparse ternary, every output |v| <= 256: bf16 stores exact,
exact zeros and pooling ties frequent) and R2 (outputs up to ~2^13: most bf16 stores round).

The entries are driven through the wrappers of model/nets.py (and the raw C-ABI where the model
calls it directly); shapes sit where launch geometry changes: 40-pixel tile columns (W = 39, 40,
41, 79, 81), block heights (H = 5..7, 11..14), odd maps, one image, narrow maps, more tiles than a
persistent grid has workgroups, reserved CUs, and two layers at the bench shape.
"""
import pytest
import torch

from tests import exact_conv as X

pytestmark = pytest.mark.gpu

CL = torch.channels_last
REGIMES = ('r1', 'r2')


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=['mfma32x32x16', 'mfma16x16x32'])
def lds_kernel(request):
    """Pins the kernel csrc/conv_lds.hip hands a call to (csrc/convg.hip: 40000 + v, csrc/convh.hip: 50000 + v)."""
    from soft_contrastive_learning_amd import _lib as L
    base = 40000 if request.param == 'mfma32x32x16' else 50000
    with L.variant(base):
        yield base


@pytest.fixture
def block_height(request, lds_kernel):
    """Pins the LDS-weights kernel's block height for one test."""
    from soft_contrastive_learning_amd import _lib as L
    with L.variant(lds_kernel + 3000 + request.param):
        yield request.param


@pytest.fixture
def reserve():
    """scl_set_reserve_cus(n) for the duration of a test."""
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    yield lambda n: lib.scl_set_reserve_cus(int(n))
    lib.scl_set_reserve_cus(0)


@pytest.fixture
def sink():
    """A gradient sink over the given parameters, as bench.py / train.py install it."""
    from soft_contrastive_learning_amd import parallel
    from soft_contrastive_learning_amd.model import nets

    def make(params):
        nets.GRAD_SINK = parallel.GradBuckets(params)
        return nets.GRAD_SINK
    yield make
    nets.GRAD_SINK = None


def _cl(t):
    return t.contiguous(memory_format=CL)


def _operands(regime, b, cin, kout, h, w, seed, dev):
    g = X.generator(seed, dev)
    make = X.r1_operands if regime == 'r1' else X.r2_operands
    x, wt = make(b, cin, kout, h, w, g, dev)
    return _cl(x), wt, g


def _fwd_ref(regime, x, wt, bias=None):
    """The exact forward (float64) after asserting the regime's premise."""
    extra = float(bias.abs().max()) if bias is not None else 0.0
    if regime == 'r1':
        X.premise(X.conv3x3, x, wt, limit=X.BF16_EXACT + 1, extra=extra)
    else:
        X.premise(X.conv3x3, x, wt, extra=extra)
    return X.conv3x3(x, wt, bias)


def _same(got, want, what):
    """torch.equal, with the count and first position of mismatches in the message."""
    want = want.to(got.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want)
    first = [int(i) for i in bad.nonzero()[0]]
    raise AssertionError('%s: %d of %d differ; first at %s: got %r want %r' % (
        what, int(bad.sum()), bad.numel(), first, float(got[tuple(first)]), float(want[tuple(first)])))


def _pool_ref(z, bias):
    """(bf16 relu(maxpool(z) + bias), window index) from the exact z."""
    m, idx = X.maxpool2x2(z)
    return X.to_bf16(torch.relu(m + bias.double()[None, :, None, None])), idx


def _ties(z):
    ho, wo = z.shape[2] // 2, z.shape[3] // 2
    win = torch.stack([z[:, :, dy:2 * ho:2, dx:2 * wo:2] for dy in (0, 1) for dx in (0, 1)], -1)
    return float(((win == win.amax(-1, keepdim=True)).sum(-1) > 1).double().mean())


def _mask_like(shape, g, dev):
    """A bf16 ReLU' mask source: positives, exact zeros, negative zeros and negatives."""
    y = X.small_ints(shape, -1, 1, g, dev, torch.float32)
    y = torch.where((y == 0) & (torch.rand(shape, generator=g, device=dev) < 0.5), -0.0, y)
    return _cl(y.to(torch.bfloat16))


# ---- forward, register-weights kernels (scl_conv3x3_fused, scl_conv3x3_pool_idx) -----------------

REG = [((64, 64), (1, 5, 39)), ((64, 64), (2, 12, 40)), ((64, 64), (1, 13, 81)), ((64, 64), (1, 2, 2)),
       ((64, 128), (1, 7, 41)), ((64, 128), (2, 6, 79)), ((128, 64), (1, 11, 40)),
       ((128, 64), (1, 14, 33)), ((128, 128), (1, 12, 79)), ((128, 128), (2, 13, 41))]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('ch,shape', REG, ids=['%dx%d-%dx%dx%d' % (c + s) for c, s in REG])
def test_register_forward(dev, regime, ch, shape):
    from soft_contrastive_learning_amd.model import nets
    (cin, kout), (b, h, w) = ch, shape
    x, wt, g = _operands(regime, b, cin, kout, h, w, 100 + cin + kout + h * w, dev)
    assert nets._own_conv_kind(x, wt) == 'reg'
    bias = X.int_bias(kout, g, dev)
    z = _fwd_ref(regime, x, wt, bias)
    z0 = X.conv3x3(x, wt)
    if regime == 'r2':
        assert X.not_bf16_fraction(z0) > 0.2
    _same(nets.conv64(x, wt, False), X.to_bf16(z0), 'conv')
    _same(nets.conv64(x, wt, False, bias=bias), X.to_bf16(z), 'conv + bias')
    _same(nets.conv64(x, wt, False, bias=bias, relu=True), X.to_bf16(torch.relu(z)), 'conv + bias + relu')
    zz, a = nets.conv64(x, wt, False, bias=bias, pool=True)
    _same(zz, X.to_bf16(z0), 'raw conv of the pooling epilogue')
    want_a, want_i = _pool_ref(z0, bias)
    _same(a, want_a, 'pooled')
    if cin == kout:
        a, idx = nets.conv_pool_idx(x, wt, bias)
        _same(a, want_a, 'pooled (index epilogue)')
        _same(idx, want_i, 'pool window index')
        if regime == 'r1' and h >= 4:
            assert _ties(z0) > 0.02


def test_register_forward_more_tiles_than_workgroups_and_reserved_cus(dev, reserve):
    """8 x 96x160 at 64 channels: several tile rounds per persistent workgroup; then the same with
    8 CUs reserved (248 workgroups, other rounds)."""
    from soft_contrastive_learning_amd.model import nets
    x, wt, g = _operands('r2', 8, 64, 64, 96, 160, 7, dev)
    bias = X.int_bias(64, g, dev)
    z0 = _fwd_ref('r2', x, wt)
    want_a, want_i = _pool_ref(z0, bias)
    for free in (0, 8):
        reserve(free)
        _same(nets.conv64(x, wt, False), X.to_bf16(z0), 'conv, reserve %d' % free)
        a, idx = nets.conv_pool_idx(x, wt, bias)
        _same(a, want_a, 'pooled, reserve %d' % free)
        _same(idx, want_i, 'index, reserve %d' % free)


# ---- forward + backward-data, LDS-weights kernels (scl_convg / convh, *_pool_idx, *_masked) ------

LDS = [(256, 256, (1, 13, 41)), (256, 128, (2, 6, 40)), (512, 512, (1, 11, 79))]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('block_height', [12, 13, 8, 6], indirect=True)
@pytest.mark.parametrize('cin,kout,shape', LDS, ids=['%dx%d-%dx%dx%d' % ((c, k) + s) for c, k, s in LDS])
def test_lds_forward_and_backward_data(dev, regime, cin, kout, shape, block_height):
    from soft_contrastive_learning_amd.model import nets
    b, h, w = shape
    x, wt, g = _operands(regime, b, cin, kout, h, w, 200 + cin + kout + h * w, dev)
    wt = _cl(wt)
    assert nets._own_conv_kind(x, wt) == 'lds'
    bias = X.int_bias(kout, g, dev)
    z = _fwd_ref(regime, x, wt, bias)
    z0 = X.conv3x3(x, wt)
    _same(nets.conv64(x, wt, False), X.to_bf16(z0), 'conv')
    _same(nets.conv64(x, wt, False, bias=bias, relu=True), X.to_bf16(torch.relu(z)), 'conv + bias + relu')
    if cin == kout:
        want_a, want_i = _pool_ref(z0, bias)
        a, idx = nets.conv_pool_idx(x, wt, bias)
        _same(a, want_a, 'pooled (index epilogue)')
        _same(idx, want_i, 'pool window index')
    # backward-data: the gradient w.r.t. x of conv(x, wt) for gy [B,kout,H,W]
    gy, _, _ = _operands(regime, b, kout, cin, h, w, 300 + cin + h, dev)
    if regime == 'r1':
        X.premise(X.conv3x3_t, gy, wt, limit=X.BF16_EXACT + 1)
    else:
        X.premise(X.conv3x3_t, gy, wt)
    gx = X.to_bf16(X.conv3x3_t(gy, wt))
    _same(nets.conv64(gy, wt, True), gx, 'backward-data')
    mask = _mask_like((b, cin, h, w), g, dev)
    _same(nets.conv64(gy, wt, True, mask=mask), torch.where(X.relu_mask(mask), gx, 0.0), 'masked backward-data')


@pytest.mark.parametrize('regime', REGIMES)
def test_lds_forward_odd_chunk_count(dev, lds_kernel, regime):
    """cin = 160: five 32-channel chunks (convh.hip walks pairs; conv_lds.hip hands these to convg.hip)."""
    from soft_contrastive_learning_amd.model import nets
    x, wt, g = _operands(regime, 1, 160, 128, 13, 41, 41, dev)
    assert nets._own_conv_kind(x, wt) == 'lds'
    bias = X.int_bias(128, g, dev)
    z = _fwd_ref(regime, x, wt, bias)
    _same(nets.conv64(x, wt, False, bias=bias, relu=True), X.to_bf16(torch.relu(z)), 'conv + bias + relu')


# The PRODUCT library's own choice (no variant: csrc/conv_lds.hip picks the kernel, the launcher the
# block height).  With 16 usable CUs and kout = 256 the 16x16x32 launcher's cost rule,
# ceil(B ceil(H / bh) ceil(W / 40) (kout / 128) / cus) (bh + 2) with ties to 12, then 8, then 6,
# gives every block height on small maps — (cin, kout, shape, height it picks, tiles the map exactly).
# The heights are by that rule (restated in _product_block_height, which checks this table), not
# observed: the library does not report its choice, so a wrong choice that computed right would pass.
# cin = 160 is five 32-channel chunks, which conv_lds.hip hands to the 32x32x16 kernel.
PRODUCT = [(256, 256, (4, 24, 40), 12, True), (256, 256, (4, 22, 38), 12, False),
           (256, 256, (4, 23, 41), 12, False), (256, 256, (4, 16, 40), 8, True),
           (256, 256, (4, 15, 40), 8, False), (256, 256, (1, 12, 40), 6, True),
           (256, 256, (1, 13, 41), 6, False), (160, 128, (1, 13, 41), None, False)]


def _product_block_height(b, h, w, kout, cus):
    cost = {bh: -(-(b * -(-h // bh) * -(-w // 40) * (kout // 128)) // cus) * (bh + 2) for bh in (12, 8, 6)}
    return min((12, 8, 6), key=lambda bh: cost[bh])           # (min keeps the first of equals)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('cin,kout,shape,bh,exact', PRODUCT, ids=['%dx%d-%dx%dx%d' % ((r[0], r[1]) + r[2]) for r in PRODUCT])
def test_lds_product_dispatch(dev, reserve, regime, cin, kout, shape, bh, exact):
    from soft_contrastive_learning_amd import _lib as L
    from soft_contrastive_learning_amd.model import nets
    assert L.load().scl_build_is_diag() == 0
    b, h, w = shape
    if bh is not None:
        assert _product_block_height(b, h, w, kout, 16) == bh and (h % bh == 0 and w % 40 == 0) == exact
    reserve(torch.cuda.get_device_properties(dev).multi_processor_count - 16)
    x, wt, g = _operands(regime, b, cin, kout, h, w, 250 + cin + h * w, dev)
    wt = _cl(wt)
    assert nets._own_conv_kind(x, wt) == 'lds'
    bias = X.int_bias(kout, g, dev)
    z = _fwd_ref(regime, x, wt, bias)
    z0 = X.conv3x3(x, wt)
    _same(nets.conv64(x, wt, False), X.to_bf16(z0), 'conv')
    _same(nets.conv64(x, wt, False, bias=bias, relu=True), X.to_bf16(torch.relu(z)), 'conv + bias + relu')
    if cin % 64:
        return                          # (its backward-data pass has 160 output channels: no LDS shape)
    if h % 2 == 0 and w % 2 == 0:
        want_a, want_i = _pool_ref(z0, bias)
        a, idx = nets.conv_pool_idx(x, wt, bias)
        _same(a, want_a, 'pooled (index epilogue)')
        _same(idx, want_i, 'pool window index')
    gy, _, _ = _operands(regime, b, kout, cin, h, w, 350 + h * w, dev)
    X.premise(X.conv3x3_t, gy, wt, limit=X.BF16_EXACT + 1 if regime == 'r1' else X.EXACT)
    gx = X.to_bf16(X.conv3x3_t(gy, wt))
    _same(nets.conv64(gy, wt, True), gx, 'backward-data')
    mask = _mask_like((b, cin, h, w), g, dev)
    _same(nets.conv64(gy, wt, True, mask=mask), torch.where(X.relu_mask(mask), gx, 0.0), 'masked backward-data')


# ---- backward-data, register kernels (scl_conv3x3 transposed, _masked, _masked_pooled) ----------

BWD = [((64, 64), (1, 6, 40)), ((64, 64), (2, 13, 41)), ((64, 64), (1, 2, 2)), ((128, 128), (1, 12, 80)),
       ((128, 128), (2, 14, 38)), ((128, 64), (1, 11, 79)), ((64, 128), (1, 5, 81))]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('ch,shape', BWD, ids=['%dx%d-%dx%dx%d' % (c + s) for c, s in BWD])
def test_register_backward_data(dev, regime, ch, shape):
    from soft_contrastive_learning_amd.model import nets
    (cin, kout), (b, h, w) = ch, shape
    # the layer is conv(cin -> kout); its backward-data pass takes gy [B,kout,H,W]
    gy, wt, g = _operands(regime, b, kout, cin, h, w, 400 + cin + kout + h * w, dev)
    wt = wt.transpose(0, 1)                                           # [kout, cin, 3, 3] view
    limit = X.BF16_EXACT + 1 if regime == 'r1' else X.EXACT
    X.premise(X.conv3x3_t, gy, wt, limit=limit)
    gx = X.to_bf16(X.conv3x3_t(gy, wt))
    _same(nets.conv64(gy, wt, True), gx, 'backward-data')
    mask = _mask_like((b, cin, h, w), g, dev)
    _same(nets.conv64(gy, wt, True, mask=mask), torch.where(X.relu_mask(mask), gx, 0.0), 'masked')
    if cin == kout and h % 2 == 0 and w % 2 == 0:
        # un-pooling while staging: gy is the gradient at the pooled map
        ga = gy[:, :, :h // 2, :w // 2].contiguous(memory_format=CL)
        idx = _cl(torch.randint(0, 4, ga.shape, generator=g, device=dev, dtype=torch.uint8))
        gz = X.unpool(ga, idx, h, w)
        X.premise(X.conv3x3_t, gz, wt, limit=limit)
        want = torch.where(X.relu_mask(mask), X.to_bf16(X.conv3x3_t(gz, wt)), 0.0)
        _same(nets.conv64(ga, wt, True, mask=mask, pool_idx=idx), want, 'masked + un-pooled')


# ---- weight gradient (scl_wrw3x3_bias, scl_wrw3x3_pooled) ---------------------------------------

WRW = [(64, 64, (1, 33, 9)), (64, 64, (2, 12, 40)), (128, 64, (1, 13, 41)), (64, 128, (2, 6, 79)),
       (256, 256, (2, 14, 80)), (512, 512, (1, 7, 23)), (128, 128, (3, 36, 80))]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('cin,kout,shape', WRW, ids=['%dx%d-%dx%dx%d' % ((c, k) + s) for c, k, s in WRW])
def test_weight_gradient(dev, regime, cin, kout, shape):
    from soft_contrastive_learning_amd.model import nets
    b, h, w = shape
    g = X.generator(500 + cin + kout + h * w, dev)
    if regime == 'r1':                  # ternary: every sum over positions is a count
        x = _cl(X.ternary((b, cin, h, w), 0.5, g, dev))
        gz = _cl(X.ternary((b, kout, h, w), 0.5, g, dev))
    else:                               # a sign per channel: sums grow with the positions
        x = _cl(X.small_ints((b, cin, h, w), 0, 3, g, dev))
        sign = torch.where(torch.rand(kout, generator=g, device=dev) < 0.5, -1.0, 1.0)
        gz = _cl((X.small_ints((b, kout, h, w), -1, 6, g, dev, torch.float32)
                  * sign[None, :, None, None]).bfloat16())
    X.premise(X.conv3x3_wgrad, x, gz)
    gw = X.conv3x3_wgrad(x, gz)
    gb = X.bias_grad(gz)
    if regime == 'r2':
        assert X.not_bf16_fraction(gw) > 0.1
    for like in (torch.empty(kout, cin, 3, 3, device=dev, dtype=torch.bfloat16),
                 torch.empty(kout, cin, 3, 3, device=dev, dtype=torch.bfloat16).contiguous(memory_format=CL),
                 torch.empty(kout, cin, 3, 3, device=dev)):
        got_b = torch.full((kout,), 7.0, device=dev)
        got = nets.wrw64(x, gz, like, got_b)
        assert got.dtype == like.dtype and got.stride() == like.stride()
        _same(got, X.to_bf16(gw) if like.dtype == torch.bfloat16 else gw.float(), 'weight gradient %s' % like.dtype)
        _same(got_b, gb.float(), 'bias gradient')
    if h % 2 == 0 and w % 2 == 0:
        ga = gz[:, :, :h // 2, :w // 2].contiguous(memory_format=CL)
        idx = _cl(torch.randint(0, 4, ga.shape, generator=g, device=dev, dtype=torch.uint8))
        gzu = X.unpool(ga, idx, h, w)
        gw = X.conv3x3_wgrad(x, gzu)
        for like in (torch.empty(kout, cin, 3, 3, device=dev, dtype=torch.bfloat16),
                     torch.empty(kout, cin, 3, 3, device=dev)):
            got_b = torch.empty(kout, device=dev)
            got = nets.wrw64(x, ga, like, got_b, pool_idx=idx)
            _same(got, X.to_bf16(gw) if like.dtype == torch.bfloat16 else gw.float(), 'pooled weight gradient')
            _same(got_b, X.bias_grad(gzu).float(), 'pooled bias gradient')


def test_weight_gradient_with_reserved_cus(dev, reserve):
    """Other weight-gradient pixel splits (248 workgroups): still exact."""
    from soft_contrastive_learning_amd.model import nets
    g = X.generator(77, dev)
    x = _cl(X.small_ints((4, 128, 30, 40), 0, 3, g, dev))
    gz = _cl(X.small_ints((4, 128, 30, 40), -3, 3, g, dev))
    X.premise(X.conv3x3_wgrad, x, gz)
    want = X.conv3x3_wgrad(x, gz).float()
    like = torch.empty(128, 128, 3, 3, device=dev)
    for free in (8, 0):
        reserve(free)
        gb = torch.empty(128, device=dev)
        _same(nets.wrw64(x, gz, like, gb), want, 'weight gradient, reserve %d' % free)
        _same(gb, X.bias_grad(gz).float(), 'bias gradient, reserve %d' % free)


# ---- weight formats: strided bf16, float32 masters halfway between bf16 values, packed images ----

@pytest.mark.parametrize('cin,kout,shape', [(64, 64, (1, 13, 41)), (128, 128, (1, 12, 40)),
                                            (256, 256, (1, 11, 39)), (128, 256, (1, 6, 81))])
def test_weight_formats(dev, cin, kout, shape):
    from soft_contrastive_learning_amd.model import nets
    b, h, w = shape
    g = X.generator(600 + cin + kout, dev)
    x = _cl(X.ternary((b, cin, h, w), 0.25, g, dev))
    gy = _cl(X.ternary((b, kout, h, w), 0.25, g, dev))
    w32 = X.halfway_master((kout, cin, 3, 3), g, dev)
    wq = w32.bfloat16()                            # round-to-nearest-even on the host side
    assert float((wq.float() != w32).double().mean()) > 0.15
    bias = X.int_bias(kout, g, dev)
    X.premise(X.conv3x3, x, wq, extra=4)
    X.premise(X.conv3x3_t, gy, wq)
    z = X.conv3x3(x, wq, bias)
    gx = X.to_bf16(X.conv3x3_t(gy, wq))
    fwd = X.to_bf16(torch.relu(z))
    # float32 master, bf16 contiguous, channels-last and a strided view of a larger tensor
    big = torch.zeros(kout, 2 * cin, 3, 3, dtype=torch.bfloat16, device=dev)
    big[:, ::2] = wq
    formats = [w32, wq, _cl(wq), big[:, ::2]]
    for i, wt in enumerate(formats):
        _same(nets.conv64(x, wt, False, bias=bias, relu=True), fwd, 'forward, format %d' % i)
        _same(nets.conv64(gy, wt, True), gx, 'backward-data, format %d' % i)
    # packed images written by one scl_conv_pack_batch launch (the model's forward pass)
    for wt in (w32, _cl(wq)):
        assert nets.prepack([wt], force=True) == 2
        assert nets._packed_for(wt, False) is not None and nets._packed_for(wt, True) is not None
        _same(nets.conv64(x, wt, False, bias=bias, relu=True), fwd, 'forward, packed %s' % wt.dtype)
        _same(nets.conv64(gy, wt, True), gx, 'backward-data, packed %s' % wt.dtype)
        if cin == kout:
            want_a, want_i = _pool_ref(X.conv3x3(x, wq), bias)
            a, idx = nets.conv_pool_idx(x, wt, bias)
            _same(a, want_a, 'pooled, packed')
            _same(idx, want_i, 'index, packed')


# ---- first layer (scl_conv_first, scl_conv_first_pool_idx, scl_conv_first_wrw, fused wrw) -------

def _first_operands(regime, b, h, w, g, dev, w_f32):
    """img float32 (integers 0..255), integer avg, conv1_1 / conv1_2 weights and biases."""
    avg = torch.tensor([124.0, 117.0, 104.0], device=dev)
    if regime == 'r1':                 # x0 = img - avg sparse in -1..1: y1 and z2 stay <= 256
        img = avg + X.ternary((b, h, w, 3), 0.5, g, dev, torch.float32)
        w1 = X.ternary((64, 3, 3, 3), 0.5, g, dev, torch.float32)
        w2 = X.ternary((64, 64, 3, 3), 0.05, g, dev, torch.float32)
    else:                              # x0 up to +-255: y1 up to ~2^14, most of it rounds
        img = torch.randint(0, 256, (b, h, w, 3), generator=g, device=dev).float()
        w1 = X.small_ints((64, 3, 3, 3), -3, 3, g, dev, torch.float32)
        w2 = X.ternary((64, 64, 3, 3), 0.01, g, dev, torch.float32)
    b1, b2 = X.int_bias(64, g, dev), X.int_bias(64, g, dev)
    if w_f32:
        w1 = torch.where(torch.rand(w1.shape, generator=g, device=dev) < 0.2, 259.0 * torch.sign(w1), w1)   # 259: halfway, RNE 260, truncation 258
    else:
        w1, w2 = _cl(w1.bfloat16()), _cl(w2.bfloat16())
    return img, avg, w1, b1, w2, b2


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('w_f32', [False, True])
@pytest.mark.parametrize('shape', [(1, 13, 41), (2, 16, 64), (1, 14, 38), (1, 6, 80)])
def test_first_layer_forward(dev, regime, w_f32, shape):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    b, h, w = shape
    g = X.generator(700 + h * w, dev)
    img, avg, w1, b1, w2, b2 = _first_operands(regime, b, h, w, g, dev, w_f32)
    w1q, w2q = w1.bfloat16(), w2.bfloat16()
    x0 = (img - avg).permute(0, 3, 1, 2)                   # exact integers
    X.premise(X.conv3x3, x0, w1q, extra=4)
    y1 = X.to_bf16(torch.relu(X.conv3x3(x0, w1q, b1)))
    if regime == 'r2':
        assert X.not_bf16_fraction(torch.relu(X.conv3x3(x0, w1q, b1))) > 0.2
    got_x0 = torch.empty((b, h, w, 3), dtype=torch.bfloat16, device=dev)
    got_y1 = torch.empty((b, h, w, 64), dtype=torch.bfloat16, device=dev)
    L.check(lib.scl_conv_first(L.ptr(img), L.ptr(avg), L.ptr(w1), *w1.stride(), int(w_f32), L.ptr(b1),
                               b, h, w, L.ptr(got_x0), L.ptr(got_y1), L.stream_of(img)))
    _same(got_x0.permute(0, 3, 1, 2), X.to_bf16(x0), 'x0')
    _same(got_y1.permute(0, 3, 1, 2), y1, 'y1')
    if h % 2 or w % 2:
        return
    X.premise(X.conv3x3, y1, w2q, extra=4)
    want_a, want_i = _pool_ref(X.conv3x3(y1, w2q), b2)
    out = [torch.full((b, h, w, 3), 7, dtype=torch.bfloat16, device=dev),
           torch.full((b, h, w, 64), 7, dtype=torch.bfloat16, device=dev),
           torch.full((b, h // 2, w // 2, 64), 7, dtype=torch.bfloat16, device=dev),
           torch.full((b, h // 2, w // 2, 64), 9, dtype=torch.uint8, device=dev)]
    ws = L.workspace(lib.scl_conv3x3_workspace_bytes(), dev)
    L.check(lib.scl_conv_first_pool_idx(L.ptr(img), L.ptr(avg), L.ptr(w1), *w1.stride(), int(w_f32),
                                        L.ptr(b1), L.ptr(w2), *w2.stride(), L.W_F32 if w_f32 else 0,
                                        L.ptr(b2), b, h, w, *[L.ptr(t) for t in out], L.ptr(ws), ws.numel(),
                                        L.stream_of(img)))
    _same(out[0].permute(0, 3, 1, 2), X.to_bf16(x0), 'x0 (two layers in one kernel)')
    _same(out[1].permute(0, 3, 1, 2), y1, 'y1 (two layers in one kernel)')
    _same(out[2].permute(0, 3, 1, 2), want_a, 'pooled (two layers in one kernel)')
    _same(out[3].permute(0, 3, 1, 2), want_i, 'index (two layers in one kernel)')


def _davg_ref(gz, wq):
    """d loss / d average_rgb = - the spatial sum of conv1_1's input gradient."""
    return -X.conv3x3_t(gz, wq).sum(dim=(0, 2, 3))


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('shape', [(1, 13, 41), (2, 16, 40), (1, 33, 9), (3, 40, 96)])
def test_first_layer_gradients(dev, regime, shape):
    """nets.first_wrw (weight, bias and mean gradient in one pass) and nets.avg_rgb_grad."""
    from soft_contrastive_learning_amd.model import nets
    b, h, w = shape
    g = X.generator(800 + h * w, dev)
    if regime == 'r1':
        x0 = X.ternary((b, h, w, 3), 0.5, g, dev)
        gz = _cl(X.ternary((b, 64, h, w), 0.5, g, dev))
    else:
        x0 = X.small_ints((b, h, w, 3), -200, 200, g, dev)
        gz = _cl(X.small_ints((b, 64, h, w), -3, 3, g, dev, density=0.25))
    x0 = x0.permute(0, 3, 1, 2)
    wq = _cl(X.small_ints((64, 3, 3, 3), -3, 3, g, dev))
    X.premise(X.conv3x3_wgrad, x0, gz)
    X.premise(lambda a, c: _davg_ref(a, c).abs(), gz, wq)
    gw, gb, davg = X.conv3x3_wgrad(x0, gz), X.bias_grad(gz).float(), _davg_ref(gz, wq).float()
    if regime == 'r2':
        assert X.not_bf16_fraction(gw) > 0.2
    for like in (torch.empty(64, 3, 3, 3, device=dev, dtype=torch.bfloat16).contiguous(memory_format=CL),
                 torch.empty(64, 3, 3, 3, device=dev)):
        got_b = torch.empty(64, device=dev)
        got, got_davg = nets.first_wrw(x0, gz, like, got_b, wq)
        _same(got, X.to_bf16(gw) if like.dtype == torch.bfloat16 else gw.float(), 'first weight gradient')
        _same(got_b, gb, 'first bias gradient')
        _same(got_davg, davg, 'mean gradient')
    _same(nets.avg_rgb_grad(gz, wq, gb), davg, 'avg_rgb_grad')


@pytest.mark.parametrize('shape', [(1, 14, 40), (2, 16, 80), (1, 6, 82)])
@pytest.mark.parametrize('w_f32', [False, True])
def test_first_block_fused_backward(dev, shape, w_f32):
    """scl_conv3x3_masked_pooled_first_wrw: conv1_2's backward-data pass (un-pooling, ReLU' of y1)
    with conv1_1's weight / bias / mean gradient on the LDS tile.  The kernel rounds the gradient
    at conv1_1's pre-activation to bf16 before it multiplies it with x0 (by design: it is what
    scl_conv_first_wrw would read from memory), so the data keep that intermediate at |v| <= 256,
    where the rounding is exact."""
    from soft_contrastive_learning_amd.model import nets
    b, h, w = shape
    g = X.generator(900 + h * w, dev)
    x0 = X.ternary((b, h, w, 3), 0.5, g, dev)                             # [B,H,W,3] storage
    y1 = _mask_like((b, 64, h, w), g, dev)
    ga = _cl(X.ternary((b, 64, h // 2, w // 2), 0.5, g, dev))
    idx = _cl(torch.randint(0, 4, ga.shape, generator=g, device=dev, dtype=torch.uint8))
    w2 = X.ternary((64, 64, 3, 3), 0.1, g, dev, torch.float32)
    w1 = X.small_ints((64, 3, 3, 3), -3, 3, g, dev, torch.float32)
    if not w_f32:
        w1, w2 = _cl(w1.bfloat16()), _cl(w2.bfloat16())
    b1 = torch.zeros(64, device=dev)
    gz2 = X.unpool(ga, idx, h, w)
    X.premise(X.conv3x3_t, gz2, w2, limit=X.BF16_EXACT + 1)
    gz1 = torch.where(X.relu_mask(y1), X.conv3x3_t(gz2, w2.bfloat16()), 0.0)
    x0n = x0.permute(0, 3, 1, 2)
    X.premise(X.conv3x3_wgrad, x0n, gz1)
    X.premise(lambda a, c: _davg_ref(a, c).abs(), gz1, w1.bfloat16())
    gw1, gb1, davg = nets._masked_pooled_first_wrw(ga, idx, w2, y1, (x0, w1, b1))
    want = X.conv3x3_wgrad(x0n, gz1)
    _same(gw1, want.float() if w_f32 else X.to_bf16(want), 'conv1_1 weight gradient')
    _same(gb1, X.bias_grad(gz1).float(), 'conv1_1 bias gradient')
    _same(davg, _davg_ref(gz1, w1.bfloat16()).float(), 'mean gradient')


# ---- glue (csrc/vgg_glue.hip) --------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('b,h,w,c', [(2, 5, 7, 64), (1, 6, 10, 128), (1, 9, 13, 512), (3, 2, 2, 64)])
def test_glue_kernels_tie_heavy(dev, dtype, b, h, w, c):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    code = L.DT_F32 if dtype == torch.float32 else L.DT_BF16
    g = X.generator(1000 + c + h * w, dev)
    z = X.small_ints((b, h, w, c), -1, 2, g, dev, dtype)                 # channels-last storage
    bias = X.int_bias(c, g, dev, -2, 2)
    zn = z.permute(0, 3, 1, 2).double()
    st = L.stream_of(z)
    ws = L.workspace(lib.scl_vgg_workspace_bytes(c), dev)
    # bias + relu in place
    y = z.clone()
    L.check(lib.scl_vgg_bias_act(L.ptr(y), code, L.ptr(bias), b * h * w, c, 1, st))
    _same(y.permute(0, 3, 1, 2), torch.relu(zn + bias.double()[None, :, None, None]), 'bias + relu')
    # pool forward
    m, idx = X.maxpool2x2(zn)
    assert _ties(zn) > 0.3
    a = torch.empty(b, h // 2, w // 2, c, dtype=dtype, device=dev)
    L.check(lib.scl_vgg_pool_fwd(L.ptr(z), code, L.ptr(bias), b, h, w, c, L.ptr(a), st))
    an = torch.relu(m + bias.double()[None, :, None, None])
    _same(a.permute(0, 3, 1, 2), an, 'pool forward')
    # pool backward: g * [a > 0] to the FIRST maximum of each window, zero elsewhere
    ga = X.small_ints((b, h // 2, w // 2, c), -3, 3, g, dev, dtype)
    gan = torch.where(an > 0, ga.permute(0, 3, 1, 2).double(), 0.0)
    want = X.unpool(gan, idx, h, w)
    gz = torch.full_like(z, 7.0)
    gb = torch.full((c,), 7.0, device=dev)
    L.check(lib.scl_vgg_pool_bwd(L.ptr(ga), L.ptr(a), L.ptr(z), code, b, h, w, c, L.ptr(gz), L.ptr(gb),
                                 L.ptr(ws), ws.numel(), st))
    _same(gz.permute(0, 3, 1, 2), want, 'pool backward')
    _same(gb, X.bias_grad(gan).float(), 'pool backward bias gradient')
    # the same routing from the stored index (bf16 maps: what the pooling epilogues feed it)
    if dtype == torch.bfloat16:
        gz.fill_(7.0)
        idx_cl = idx.permute(0, 2, 3, 1).contiguous()
        L.check(lib.scl_vgg_pool_bwd_idx(L.ptr(ga), L.ptr(a), L.ptr(idx_cl), code, b, h, w, c, L.ptr(gz),
                                         L.ptr(gb), L.ptr(ws), ws.numel(), st))
        _same(gz.permute(0, 3, 1, 2), want, 'pool backward by index')
        _same(gb, X.bias_grad(gan).float(), 'pool backward by index, bias gradient')
    # relu backward + bias gradient, masked by y (exact zeros included)
    gy = X.small_ints((b, h, w, c), -3, 3, g, dev, dtype)
    gz2 = torch.empty_like(gy)
    L.check(lib.scl_vgg_act_bwd(L.ptr(gy), L.ptr(y), code, b * h * w, c, L.ptr(gz2), L.ptr(gb),
                                L.ptr(ws), ws.numel(), st))
    want_g = torch.where(y > 0, gy, torch.zeros_like(gy)).permute(0, 3, 1, 2)
    _same(gz2.permute(0, 3, 1, 2), want_g, 'relu backward')
    _same(gb, X.bias_grad(want_g).float(), 'relu backward bias gradient')


# ---- two layers at the bench shape, through the dispatch VGG16NetVLAD.features takes -------------

def test_first_block_at_bench_shape(dev, sink):
    """conv1_1 -> ReLU -> conv1_2 -> pool -> ReLU at 24 x 480x640 as the model builds it (packed
    float32 master weights, the pool-index epilogue, the fused conv1_2 backward-data + conv1_1
    parameter-gradient kernel next to the weight-gradient kernel on the second stream, gradients
    in the sink).  R1 data throughout: the fused kernel rounds the gradient at conv1_1's
    pre-activation to bf16 (see test_first_block_fused_backward)."""
    from soft_contrastive_learning_amd.model import nets
    assert nets.USE_FUSED_FIRST_WRW is None and nets.USE_SIDE_WRW and nets.USE_POOL_IDX
    b, h, w = 24, 480, 640
    g = X.generator(1234, dev)
    avg0 = torch.tensor([124.0, 117.0, 104.0], device=dev)
    img = avg0 + X.ternary((b, h, w, 3), 0.5, g, dev, torch.float32)
    avg = torch.nn.Parameter(avg0.clone())
    w1 = torch.nn.Parameter(X.ternary((64, 3, 3, 3), 0.1, g, dev, torch.float32))
    b1 = torch.nn.Parameter(X.int_bias(64, g, dev, -1, 1))
    w2 = torch.nn.Parameter(X.ternary((64, 64, 3, 3), 0.05, g, dev, torch.float32))
    b2 = torch.nn.Parameter(X.int_bias(64, g, dev, -1, 1))
    buckets = sink([avg, w1, b1, w2, b2])
    assert nets.prepack([w2], force=True) == 2
    l1, l2 = nets._GradLink(), nets._GradLink()
    y1 = nets._FirstConv.apply(img, avg, w1, b1, torch.bfloat16, l1)
    a = nets._ConvBiasPoolReLU.apply(y1, w2, b2, l1, l2)
    assert a.grad_fn.by_idx and l1.first is not None
    idx = a.grad_fn.saved_tensors[2]
    x0 = (img - avg0).permute(0, 3, 1, 2)
    X.premise(X.conv3x3, x0, w1.detach(), limit=X.BF16_EXACT + 1, extra=1)
    want_y1 = X.to_bf16(torch.relu(X.conv3x3(x0, w1.detach(), b1.detach(), out_dtype=torch.float32)))
    _same(y1.detach(), want_y1, 'y1')
    X.premise(X.conv3x3, want_y1, w2.detach(), limit=X.BF16_EXACT + 1, extra=1)
    want_a, want_i = _pool_ref(X.conv3x3(want_y1, w2.detach(), out_dtype=torch.float32), b2.detach())
    _same(a.detach(), want_a, 'pooled')
    _same(idx, want_i, 'pool window index')
    ga = _cl(X.ternary(tuple(a.shape), 0.01, g, dev))
    ga = torch.where(a.detach() > 0, ga, torch.zeros_like(ga)).contiguous(memory_format=CL)
    l2.mark(ga)
    buckets.zero()
    a.backward(ga)
    buckets.finish()
    torch.cuda.synchronize()
    gz2 = X.unpool(ga, want_i, h, w)
    X.premise(X.conv3x3_wgrad, want_y1, gz2)
    _same(w2.grad, X.conv3x3_wgrad(want_y1, gz2).float(), 'conv1_2 weight gradient')
    _same(b2.grad, X.bias_grad(gz2).float(), 'conv1_2 bias gradient')
    X.premise(X.conv3x3_t, gz2, w2.detach(), limit=X.BF16_EXACT + 1)
    gz1 = torch.where(X.relu_mask(want_y1), X.conv3x3_t(gz2, w2.detach(), out_dtype=torch.float32), 0.0)
    del gz2
    X.premise(X.conv3x3_wgrad, x0, gz1)
    X.premise(lambda u, v: _davg_ref(u, v).abs(), gz1, w1.detach())
    _same(w1.grad, X.conv3x3_wgrad(x0, gz1).float(), 'conv1_1 weight gradient')
    _same(b1.grad, X.bias_grad(gz1).float(), 'conv1_1 bias gradient')
    _same(avg.grad, _davg_ref(gz1, w1.detach()).float(), 'mean gradient')


@pytest.mark.parametrize('regime', REGIMES)
def test_conv4_2_at_bench_shape(dev, sink, regime):
    """conv4_2 (512 -> 512, ReLU) at 24 x 60x80: more tiles than the persistent grids have
    workgroups; forward with bias + ReLU, masked backward-data, weight and bias gradient on the
    second stream into the sink."""
    from soft_contrastive_learning_amd.model import nets
    b, cin, kout, h, w = 24, 512, 512, 60, 80
    x, wq, g = _operands(regime, b, cin, kout, h, w, 4242, dev)
    x.requires_grad_(True)
    wt = torch.nn.Parameter(wq.float())
    bias = torch.nn.Parameter(X.int_bias(kout, g, dev))
    buckets = sink([wt, bias])
    assert nets.prepack([wt], force=True) == 2
    link_in, link_out = nets._GradLink(), nets._GradLink()
    y = nets._ConvBiasAct.apply(x, wt, bias, True, link_in, link_out)
    z = _fwd_ref(regime, x.detach(), wq, bias.detach())
    want_y = X.to_bf16(torch.relu(z))
    del z
    _same(y.detach(), want_y, 'forward')
    gy = _cl(X.ternary(tuple(y.shape), 0.5 if regime == 'r1' else 1.0, g, dev))
    gy = torch.where(want_y > 0, gy, torch.zeros_like(gy)).contiguous(memory_format=CL)
    link_out.mark(gy)
    buckets.zero()
    y.backward(gy)
    buckets.finish()
    torch.cuda.synchronize()
    assert link_in.ptr is not None
    X.premise(X.conv3x3_t, gy, wq, limit=X.BF16_EXACT + 1 if regime == 'r1' else X.EXACT)
    gx = torch.where(X.relu_mask(x.detach()), X.to_bf16(X.conv3x3_t(gy, wq, out_dtype=torch.float32)), 0.0)
    _same(x.grad, gx, 'masked backward-data')
    X.premise(X.conv3x3_wgrad, x.detach(), gy)
    _same(wt.grad, X.conv3x3_wgrad(x.detach(), gy).float(), 'weight gradient')
    _same(bias.grad, X.bias_grad(gy).float(), 'bias gradient')

"""The workspaces of the register-weights convolution family (csrc/conv64.hip, conv_wrw.hip), between guard bands.

Every workspace-taking entry point gets EXACTLY the bytes its size query returns, inside a larger
buffer whose 4096 bytes on either side must come back untouched (tests/util_guard.py), and every
output of a run on a workspace full of 0xA5 must be bit-equal to a run on a zeroed one: nothing is
read before it is written.  The shapes are the smallest with partial tiles in both directions
(2 x 10 x 36: 8- and 4-row tiles of 32 columns; 2 x 32 x 8: the weight gradient's tall tiles)."""
import pytest
import torch

from tests.util_guard import FILL, Guarded

pytestmark = pytest.mark.gpu

B, H, W = 2, 10, 36
REG = [(64, 64), (64, 128), (128, 64), (128, 128)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf16(shape, seed, dev, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).to(torch.bfloat16).to(dev)


def _f32(shape, seed, dev):
    return torch.randn(shape, generator=_gen(seed)).to(dev)


def _index(shape, seed, dev):
    return torch.randint(0, 4, shape, generator=_gen(seed), dtype=torch.uint8).to(dev)


def _sentinel(shape, dtype, dev):
    return torch.full(shape, 7, dtype=dtype, device=dev)


class _Spaces:
    """ws(nbytes) -> (pointer, nbytes) of a fresh guarded workspace; check() looks at all bands."""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.made = dev, fill, []

    def __call__(self, nbytes):
        from soft_contrastive_learning_amd import _lib as L
        g = Guarded(self.dev, nbytes, self.fill)
        self.made.append(g)
        return L.ptr(g.inner), nbytes

    def check(self):
        assert self.made
        for g in self.made:
            g.assert_bands_intact()


def _twice(dev, route):
    """route(ws) -> outputs, on workspaces full of FILL and on zeroed ones."""
    runs = []
    for fill in (FILL, 0):
        ws = _Spaces(dev, fill)
        outs = route(ws)
        ws.check()
        runs.append(outs)
    assert len(runs[0]) == len(runs[1]) > 0
    for a, b in zip(*runs):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _weight(wt, transposed, cin, kout, packed, dev):
    """(pointer, flag word, what must stay alive) of the raw weight or of its packed image."""
    from soft_contrastive_learning_amd import _lib as L
    if not packed:
        return L.ptr(wt), int(transposed), wt
    lib = L.load()
    image = torch.empty(lib.scl_conv_packed_bytes(cin, kout), dtype=torch.uint8, device=dev)
    job = (L.PackJob * 1)(L.PackJob(L.ptr(wt), *wt.stride(), int(transposed), cin, kout, L.ptr(image)))
    L.check(lib.scl_conv_pack_batch(job, 1, L.stream_of(wt)))
    torch.cuda.synchronize()
    return L.ptr(image), int(transposed) | L.W_PACKED, image


# ---- the convolution: scl_conv3x3_fused / _pool_idx / _masked / _masked_pooled -------------------

FORMS = ['plain', 'bias_relu', 'pooled', 'pool_idx', 'masked', 'masked_pooled']
CONV = [(ch, form, False) for ch in REG for form in FORMS if form != 'masked_pooled' or ch[0] == ch[1]]
CONV += [((64, 64), form, True) for form in FORMS]          # ... and with a pre-packed image


@pytest.mark.parametrize('ch,form,packed', CONV,
                         ids=['%dx%d-%s%s' % (c + (f, '-packed' if p else '')) for c, f, p in CONV])
def test_convolution_workspace_between_guard_bands(dev, ch, form, packed):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    cin, kout = ch
    transposed = form in ('masked', 'masked_pooled')
    xs = (B, H // 2, W // 2, cin) if form == 'masked_pooled' else (B, H, W, cin)
    x = _bf16(xs, 1, dev)
    wt = _bf16((cin, kout, 3, 3) if transposed else (kout, cin, 3, 3), 2, dev, 0.1)
    bias, mask, uidx = _f32((kout,), 3, dev), _bf16((B, H, W, kout), 4, dev), _index(xs, 5, dev)
    wp, flags, alive = _weight(wt, transposed, cin, kout, packed, dev)
    st = L.stream_of(x)

    def route(ws):
        out = _sentinel((B, H, W, kout), torch.bfloat16, dev)
        pooled = _sentinel((B, H // 2, W // 2, kout), torch.bfloat16, dev)
        pidx = _sentinel((B, H // 2, W // 2, kout), torch.uint8, dev)
        wsp, n = ws(lib.scl_conv3x3_workspace_bytes())
        head = (wp,) + tuple(wt.stride())
        if form in ('plain', 'bias_relu', 'pooled'):
            tail = {'plain': (None, 0, None), 'bias_relu': (L.ptr(bias), 1, None),
                    'pooled': (L.ptr(bias), 0, L.ptr(pooled))}[form]
            L.check(lib.scl_conv3x3_fused(L.ptr(x), *head, flags, B, H, W, cin, kout, L.ptr(out), *tail, wsp, n,
                                          st))
            return [out, pooled] if form == 'pooled' else [out]
        if form == 'pool_idx':
            L.check(lib.scl_conv3x3_pool_idx(L.ptr(x), *head, flags, B, H, W, cin, kout, L.ptr(bias),
                                             L.ptr(pooled), L.ptr(pidx), wsp, n, st))
            return [pooled, pidx]
        if form == 'masked':
            L.check(lib.scl_conv3x3_masked(L.ptr(x), *head, flags, B, H, W, cin, kout, L.ptr(out), L.ptr(mask),
                                           wsp, n, st))
            return [out]
        L.check(lib.scl_conv3x3_masked_pooled(L.ptr(x), L.ptr(uidx), *head, flags, B, H, W, cin, kout, L.ptr(out),
                                              L.ptr(mask), wsp, n, st))
        return [out]

    _twice(dev, route)
    del alive


# ---- the weight gradient: scl_wrw3x3_bias (with and without the bias gradient), scl_wrw3x3_pooled ---
# 64 -> 64: [64 c] x [64 k] blocks (nkb = 1), 64 -> 128: [64 c] x [128 k] (nkb = 2).  2 x 10 x 36 takes the
# wide tiles at nkb = 1 and the tall ones at nkb = 2 (16 x 8 pads it less), 2 x 32 x 8 the tall ones, and
# 2 x 6 x 36 the wide ones at nkb = 2.
WRW = [(s, ch, form) for s in ((2, 10, 36), (2, 32, 8)) for ch in ((64, 64), (64, 128))
       for form in ('bias', 'no_bias', 'pooled')] + [((2, 6, 36), (64, 128), 'bias')]


@pytest.mark.parametrize('shape,ch,form', WRW, ids=['%dx%dx%d-%dx%d-%s' % (s + c + (f,)) for s, c, f in WRW])
def test_weight_gradient_workspace_between_guard_bands(dev, shape, ch, form):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    (b, h, w), (cin, kout) = shape, ch
    x = _bf16((b, h, w, cin), 11, dev)
    gz = _bf16((b, h // 2, w // 2, kout) if form == 'pooled' else (b, h, w, kout), 12, dev)
    idx = _index((b, h // 2, w // 2, kout), 13, dev)
    st = L.stream_of(x)

    def route(ws):
        gw = _sentinel((kout, cin, 3, 3), torch.bfloat16, dev)
        gb = None if form == 'no_bias' else _sentinel((kout,), torch.float32, dev)
        wsp, n = ws(lib.scl_wrw3x3_workspace_bytes(cin, kout))
        if form == 'pooled':
            L.check(lib.scl_wrw3x3_pooled(L.ptr(x), L.ptr(gz), L.ptr(idx), b, h, w, cin, kout, L.ptr(gw),
                                          *gw.stride(), 0, L.ptr(gb), wsp, n, st))
        else:
            L.check(lib.scl_wrw3x3_bias(L.ptr(x), L.ptr(gz), b, h, w, cin, kout, L.ptr(gw), *gw.stride(), 0,
                                        L.ptr(gb), wsp, n, st))
        return [gw] if gb is None else [gw, gb]

    _twice(dev, route)


# ---- the first layer: scl_conv_first_pool_idx, scl_conv_first_wrw, the fused backward ----------------

@pytest.mark.parametrize('packed', [False, True], ids=['raw', 'packed'])
def test_first_block_forward_workspace_between_guard_bands(dev, packed):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    img = torch.randint(0, 256, (B, H, W, 3), generator=_gen(21)).float().to(dev)
    avg = torch.tensor([124.0, 117.0, 104.0], device=dev)
    w1, b1 = _bf16((64, 3, 3, 3), 22, dev, 0.1), _f32((64,), 23, dev)
    w2, b2 = _bf16((64, 64, 3, 3), 24, dev, 0.1), _f32((64,), 25, dev)
    wp, flags, alive = _weight(w2, False, 64, 64, packed, dev)

    def route(ws):
        outs = [_sentinel((B, H, W, 3), torch.bfloat16, dev), _sentinel((B, H, W, 64), torch.bfloat16, dev),
                _sentinel((B, H // 2, W // 2, 64), torch.bfloat16, dev),
                _sentinel((B, H // 2, W // 2, 64), torch.uint8, dev)]
        wsp, n = ws(lib.scl_conv3x3_workspace_bytes())
        L.check(lib.scl_conv_first_pool_idx(L.ptr(img), L.ptr(avg), L.ptr(w1), *w1.stride(), 0, L.ptr(b1), wp,
                                            *w2.stride(), flags, L.ptr(b2), B, H, W, *[L.ptr(t) for t in outs],
                                            wsp, n, L.stream_of(img)))
        return outs

    _twice(dev, route)
    del alive


def test_first_layer_gradient_workspace_between_guard_bands(dev):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    x0, gz = _bf16((B, H, W, 3), 31, dev, 50.0), _bf16((B, H, W, 64), 32, dev)
    w1 = _bf16((64, 3, 3, 3), 33, dev, 0.1)

    def route(ws):
        gw, gb = _sentinel((64, 3, 3, 3), torch.bfloat16, dev), _sentinel((64,), torch.float32, dev)
        davg = _sentinel((3,), torch.float32, dev)
        assert gw.stride() == w1.stride()
        wsp, n = ws(lib.scl_conv_first_wrw_workspace_bytes())
        L.check(lib.scl_conv_first_wrw(L.ptr(x0), L.ptr(gz), B, H, W, L.ptr(gw), *gw.stride(), 0, L.ptr(gb),
                                       L.ptr(w1), L.ptr(davg), wsp, n, L.stream_of(gz)))
        return [gw, gb, davg]

    _twice(dev, route)


@pytest.mark.parametrize('packed', [False, True], ids=['raw', 'packed'])
def test_first_block_fused_backward_workspaces_between_guard_bands(dev, packed):
    from soft_contrastive_learning_amd import _lib as L
    lib = L.load()
    ga, idx = _bf16((B, H // 2, W // 2, 64), 41, dev), _index((B, H // 2, W // 2, 64), 42, dev)
    w2, y1 = _bf16((64, 64, 3, 3), 43, dev, 0.1), _bf16((B, H, W, 64), 44, dev)
    x0, w1 = _bf16((B, H, W, 3), 45, dev, 50.0), _bf16((64, 3, 3, 3), 46, dev, 0.1)
    wp, flags, alive = _weight(w2, True, 64, 64, packed, dev)
    flags &= ~L.CONV_TRANSPOSED            # (the entry point is a backward-data pass by itself)

    def route(ws):
        gw, gb = _sentinel((64, 3, 3, 3), torch.bfloat16, dev), _sentinel((64,), torch.float32, dev)
        davg = _sentinel((3,), torch.float32, dev)
        wsp, n = ws(lib.scl_conv3x3_workspace_bytes())
        fwp, fn = ws(lib.scl_conv_first_wrw_workspace_bytes())
        L.check(lib.scl_conv3x3_masked_pooled_first_wrw(
            L.ptr(ga), L.ptr(idx), wp, *w2.stride(), flags, B, H, W, L.ptr(y1), L.ptr(x0), L.ptr(gw),
            *gw.stride(), 0, L.ptr(gb), L.ptr(w1), L.ptr(davg), wsp, n, fwp, fn, L.stream_of(ga)))
        return [gw, gb, davg]

    _twice(dev, route)
    del alive

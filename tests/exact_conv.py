"""Exact references for the backbone's 3x3 convolutions, built from taps in float64.

The own convolution kernels accumulate in float32 and round once to bf16.  With small-integer
operands every product is exact, and while every partial sum is an integer below 2^24 the float32
accumulation is exact in ANY summation order: the kernel's result must then equal these references
bit for bit (bf16 outputs: the exact value rounded once, to nearest even), and the discrete
decisions that follow from it — the ReLU mask, the max-pool window index under ties — can be
checked too.  ``premise`` asserts that bound for the data of a test.

Everything here computes in float64 on the device of its inputs, as sums of nine shifted slices
contracted over channels (no library convolution: its algorithm choice is not exact); results may
be returned in float32, which holds every integer below 2^24 exactly.  Tensors are NCHW in shape
(channels-last storage is fine).
"""
import torch
import torch.nn.functional as F

EXACT = 2 ** 24                        # float32 integers are exact below this
BF16_EXACT = 256                       # ... bf16 integers up to this magnitude


def _chunks(b, per_image, budget=1 << 26):
    """Image ranges whose float64 working set stays near ``budget`` elements."""
    step = max(1, budget // max(1, per_image))
    return [(lo, min(b, lo + step)) for lo in range(0, b, step)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).double()


def conv3x3(x, w, bias=None, out_dtype=torch.float64):
    """'same' 3x3 convolution: out[b,k,y,x] = sum_{c,kh,kw} x[b,c,y+kh-1,x+kw-1] w[k,c,kh,kw]
    (+ bias[k]).  x [B,C,H,W], w [K,C,3,3] -> [B,K,H,W] ``out_dtype``."""
    b, c, h, wd = x.shape
    k = w.shape[0]
    taps = w.double().permute(2, 3, 1, 0)                                # [3,3,C,K]
    out = torch.empty((b, k, h, wd), dtype=out_dtype, device=x.device)
    for lo, hi in _chunks(b, (h + 2) * (wd + 2) * c + 2 * h * wd * k):
        xp = F.pad(_nhwc(x[lo:hi]), (0, 0, 1, 1, 1, 1))                   # [n,H+2,W+2,C]
        acc = torch.zeros((hi - lo, h, wd, k), dtype=torch.float64, device=x.device)
        for kh in range(3):
            for kw in range(3):
                acc += xp[:, kh:kh + h, kw:kw + wd, :] @ taps[kh, kw]
        if bias is not None:
            acc += bias.double()
        out[lo:hi] = acc.permute(0, 3, 1, 2).to(out_dtype)
    return out


def conv3x3_t(gz, w, out_dtype=torch.float64):
    """Gradient w.r.t. the input of conv3x3(., w) for the output gradient gz [B,K,H,W]:
    gx[b,c,y,x] = sum_{k,kh,kw} gz[b,k,y+1-kh,x+1-kw] w[k,c,kh,kw] -> [B,C,H,W]."""
    b, k, h, wd = gz.shape
    c = w.shape[1]
    taps = w.double().permute(2, 3, 0, 1)                                # [3,3,K,C]
    out = torch.empty((b, c, h, wd), dtype=out_dtype, device=gz.device)
    for lo, hi in _chunks(b, (h + 2) * (wd + 2) * k + 2 * h * wd * c):
        gp = F.pad(_nhwc(gz[lo:hi]), (0, 0, 1, 1, 1, 1))
        acc = torch.zeros((hi - lo, h, wd, c), dtype=torch.float64, device=gz.device)
        for kh in range(3):
            for kw in range(3):
                acc += gp[:, 2 - kh:2 - kh + h, 2 - kw:2 - kw + wd, :] @ taps[kh, kw]
        out[lo:hi] = acc.permute(0, 3, 1, 2).to(out_dtype)
    return out


def conv3x3_wgrad(x, gz):
    """Weight gradient of conv3x3(x, w) for the output gradient gz: gw[k,c,kh,kw] =
    sum_{b,y,x} gz[b,k,y,x] x[b,c,y+kh-1,x+kw-1] -> float64 [K,C,3,3]."""
    b, c, h, wd = x.shape
    k = gz.shape[1]
    gw = torch.zeros((3, 3, k, c), dtype=torch.float64, device=x.device)
    for lo, hi in _chunks(b, (h + 2) * (wd + 2) * c + h * wd * (k + c)):
        xp = F.pad(_nhwc(x[lo:hi]), (0, 0, 1, 1, 1, 1))
        g = _nhwc(gz[lo:hi]).reshape(-1, k).t()                            # [K, n*H*W]
        for kh in range(3):
            for kw in range(3):
                gw[kh, kw] += g @ xp[:, kh:kh + h, kw:kw + wd, :].reshape(-1, c)
    return gw.permute(2, 3, 0, 1).contiguous()


def bias_grad(gz):
    """Column sums of gz [B,K,H,W] -> float64 [K]."""
    b, k, h, wd = gz.shape
    out = torch.zeros(k, dtype=torch.float64, device=gz.device)
    for lo, hi in _chunks(b, h * wd * k):
        out += gz[lo:hi].double().sum(dim=(0, 2, 3))
    return out


def maxpool2x2(z):
    """2x2 / stride 2 'valid' max-pool of z [B,C,H,W] -> (max, idx uint8) of [B,C,H/2,W/2]; idx
    is the window position 2 dy + dx of the FIRST maximum in raster order (0,0), (0,1), (1,0),
    (1,1) — what max_pool2d's argmax picks and what the kernels document."""
    ho, wo = z.shape[2] // 2, z.shape[3] // 2
    win = [z[:, :, dy:2 * ho:2, dx:2 * wo:2] for dy in (0, 1) for dx in (0, 1)]
    m = torch.maximum(torch.maximum(win[0], win[1]), torch.maximum(win[2], win[3]))
    idx = torch.full(m.shape, 3, dtype=torch.uint8, device=z.device)
    for k in (2, 1, 0):                                   # the lowest position that holds m wins
        idx = torch.where(win[k] == m, torch.full_like(idx, k), idx)
    return m, idx


def unpool(g, idx, h, w, dtype=None):
    """The full-size [B,C,h,w] map with g at the window position idx of every pooled element and
    zero elsewhere (uncovered borders of odd maps included)."""
    b, c, ho, wo = g.shape
    out = torch.zeros((b, c, h, w), dtype=dtype or g.dtype, device=g.device)
    for k in range(4):
        out[:, :, (k >> 1):2 * ho:2, (k & 1):2 * wo:2] = torch.where(idx == k, g, torch.zeros_like(g))
    return out


def relu_mask(y):
    """ReLU' of a layer whose output is y: [y > 0] (exact zeros and -0 cut)."""
    return y > 0


def to_bf16(v):
    """The exact value ``v`` (an integer below 2^24 in magnitude) rounded ONCE to bf16, to nearest
    even: float64 -> float32 is exact there, float32 -> bf16 is torch's round-to-nearest-even."""
    return v.float().to(torch.bfloat16)


def premise(fn, *args, limit=EXACT, extra=0.0):
    """Asserts that ``fn`` (one of the contractions above) of the magnitudes of ``args`` stays
    below ``limit`` everywhere (``extra``: a bias magnitude added on top).  Every partial sum a
    kernel can form is bounded by it, so for integer data below 2^24 the float32 accumulation is
    exact in any order.  Returns the bound."""
    bound = float(fn(*(a.abs() for a in args)).max()) + float(extra)
    assert bound < limit, ("exactness premise violated", bound, limit)
    return bound


def not_bf16_fraction(v):
    """Fraction of the values that a bf16 store must round."""
    return float((v.float().to(torch.bfloat16).float() != v.float()).float().mean())


# ---- data --------------------------------------------------------------------------------------

def generator(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def ternary(shape, density, gen, device, dtype=torch.bfloat16):
    """Values in {-1, 0, 1}, each non-zero with probability ``density`` (signs even)."""
    r = torch.rand(shape, generator=gen, device=device)
    v = torch.where(r < 0.5 * density, -1.0, torch.where(r < density, 1.0, 0.0))
    return v.to(dtype)


def small_ints(shape, lo, hi, gen, device, dtype=torch.bfloat16, density=1.0):
    """Integers uniform in [lo, hi], each kept with probability ``density`` (else 0)."""
    v = torch.randint(lo, hi + 1, shape, generator=gen, device=device).float()
    if density < 1.0:
        v = torch.where(torch.rand(shape, generator=gen, device=device) < density, v, 0.0)
    return v.to(dtype)


def r1_operands(b, cin, kout, h, w, gen, device, target=16.0):
    """Regime R1 ("small"): sparse ternary activations and weights with about ``target`` non-zero
    products per output, so every output is a small integer (|v| <= 256 is asserted by the
    caller's premise): bf16 stores are exact, exact zeros and pooling ties are frequent.
    Returns x [B,cin,H,W] bf16 (channels-last), w [kout,cin,3,3] bf16."""
    dx = 0.5
    dw = min(1.0, target / (9.0 * cin * dx))
    x = ternary((b, h, w, cin), dx, gen, device).permute(0, 3, 1, 2)
    wt = ternary((kout, cin, 3, 3), dw, gen, device)
    return x, wt


def r2_operands(b, cin, kout, h, w, gen, device):
    """Regime R2 ("large"): activations in 0..3 (post-ReLU-like), weights of magnitude <= 3 with a
    sign per output channel, so outputs run to about 9 * cin * 1.5 (2^13 at cin = 512, bounded by
    9 * cin * 9 < 2^16): most bf16 stores must round — to nearest even."""
    x = small_ints((b, h, w, cin), 0, 3, gen, device).permute(0, 3, 1, 2)
    sign = torch.where(torch.rand(kout, generator=gen, device=device) < 0.5, -1.0, 1.0)
    wt = (small_ints((kout, cin, 3, 3), -1, 3, gen, device, torch.float32)
          * sign[:, None, None, None]).to(torch.bfloat16)
    return x, wt


def halfway_master(shape, gen, device, frac=0.25):
    """float32 master weights: small integers in -3..3, a ``frac`` of them replaced by values
    exactly halfway between two bf16 neighbours — odd integers in +-[257, 511] (the bf16 spacing
    there is 2) — so the in-kernel cast must round to nearest EVEN to give ``.bfloat16()``."""
    base = small_ints(shape, -3, 3, gen, device, torch.float32)
    odd = 2.0 * torch.randint(128, 256, shape, generator=gen, device=device).float() + 1.0   # 257..511
    sign = torch.where(torch.rand(shape, generator=gen, device=device) < 0.5, -1.0, 1.0)
    pick = torch.rand(shape, generator=gen, device=device) < frac
    return torch.where(pick, odd * sign, base).contiguous()


def int_bias(k, gen, device, lo=-4, hi=4):
    """A float32 bias of small integers (the epilogue's f32 add stays exact)."""
    return torch.randint(lo, hi + 1, (k,), generator=gen, device=device).float()

"""Host-side checks of the match saliency (no GPU): the grad_nets hook on a CPU model, the NumPy
statement of the contract in evaluation/saliency.py on constructed cases with known answers, the
axis tables against a float64 restatement written out here, and the two C-ABI additions of
include/scl_hip.h (bound, validation before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

NULL, SHAPE, KIND = -3, -1, -2
NEW = ("scl_saliency_map", "scl_saliency_overlay")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


# ---- the hook -------------------------------------------------------------------------------------

def test_grad_nets_imports_and_is_reachable_as_learnlarge():
    import sys
    import soft_contrastive_learning_amd as scl
    from soft_contrastive_learning_amd.model import grad_nets
    assert callable(grad_nets.vgg16Netvlad) and callable(grad_nets.vgg16)
    saved = {k: v for k, v in sys.modules.items() if k.split('.')[0] in ('learnlarge', 'pointnetvlad', 'pointnetvlad_cls')}
    try:
        pkg = scl.install_as_learnlarge()
        import learnlarge.model.grad_nets as aliased
        assert aliased is grad_nets and pkg.model.grad_nets is grad_nets
        assert sys.modules['learnlarge.model.nets'] is sys.modules['soft_contrastive_learning_amd.model.nets']
    finally:
        for k in [k for k in sys.modules if k.split('.')[0] in ('learnlarge', 'pointnetvlad', 'pointnetvlad_cls')]:
            del sys.modules[k]
        sys.modules.update(saved)


def _cpu_model(vlad_cores):
    from soft_contrastive_learning_amd.model import nets
    return nets.VGG16NetVLAD(fused_relu=False, vlad_cores=vlad_cores)


def _images():
    return torch.randint(0, 256, (2, 32, 48, 3), generator=torch.Generator().manual_seed(7)).float()


def test_vgg16_hook_on_a_cpu_model():
    from soft_contrastive_learning_amd.model import grad_nets, nets
    model, img = _cpu_model(0), _images()
    with torch.no_grad():
        want = nets.vgg16(img, model=model)
    first, grad_in = grad_nets.vgg16(img, model=model)
    assert torch.equal(first.detach(), want)
    assert tuple(grad_in.shape) == (2, 2, 3, 512) and grad_in.dtype == torch.float32
    weights = torch.randn(first.shape, generator=torch.Generator().manual_seed(1))
    (g,) = torch.autograd.grad((first * weights).sum(), grad_in)
    assert g.shape == grad_in.shape and torch.isfinite(g).all() and float(g.abs().sum()) > 0
    assert all(p.grad is None for p in model.parameters())
    # behind the channel L2 norm a position's vector may be scaled freely: gradient x activation
    # sums to zero over the channels (why no such mode exists)
    ga = (g * grad_in.detach()).sum(-1)
    assert float(ga.abs().max()) <= 1e-4 * float((g.abs() * grad_in.detach().abs()).sum(-1).max())
    # cut: the same first value, grad_in a leaf that the backbone's graph does not hang on
    first_c, leaf = grad_nets.vgg16(img, model=model, cut=True)
    assert torch.equal(first_c.detach(), want) and leaf.is_leaf and leaf.requires_grad
    (gc,) = torch.autograd.grad((first_c * weights).sum(), leaf)
    assert torch.equal(gc, g)


def test_vgg16netvlad_hook_on_a_cpu_model():
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.model import grad_nets, nets
    model, img = _cpu_model(64), _images()
    try:
        desc, grad_in = grad_nets.vgg16Netvlad(img, model=model)
    except _lib.SclError:
        pytest.skip('the NetVLAD head needs a HIP device (no CPU fallback exists)')
    with torch.no_grad():
        assert torch.equal(desc.detach(), nets.vgg16Netvlad(img, model=model))
    assert tuple(grad_in.shape) == (2, 2, 3, 512)


# ---- upsample_plan ----------------------------------------------------------------------------------

def _plan_restated(src, dst):
    i0s, i1s, ts = [], [], []
    for j in range(dst):
        f = (j + 0.5) * src / dst - 0.5
        f = min(max(f, 0.0), float(src - 1))
        i0 = math.floor(f)
        i0s.append(i0)
        i1s.append(min(i0 + 1, src - 1))
        ts.append(np.float32(f - i0))
    return np.array(i0s, np.int32), np.array(i1s, np.int32), np.array(ts, np.float32)


def test_upsample_plan():
    from soft_contrastive_learning_amd.evaluation.saliency import upsample_plan
    for n in (1, 2, 7, 15):                                            # identity
        i0, i1, t = upsample_plan(n, n)
        assert i0.dtype == np.int32 and i1.dtype == np.int32 and t.dtype == np.float32
        assert i0.tolist() == list(range(n)) and (t == 0).all()
    i0, i1, t = upsample_plan(1, 9)                                    # one sample: a constant
    assert (i0 == 0).all() and (i1 == 0).all() and (t == 0).all()
    for src, dst in ((3, 7), (15, 240), (11, 180), (9, 4), (7, 5), (2, 3)):
        got, want = upsample_plan(src, dst), _plan_restated(src, dst)
        for a, b in zip(got, want):
            assert a.shape == (dst,) and np.array_equal(a, b), (src, dst)
        i0, i1, t = got
        assert i0.min() >= 0 and i1.max() <= src - 1 and (i1 >= i0).all() and (i1 - i0 <= 1).all()
        assert (t >= 0).all() and (t < 1).all()
    # 3 -> 7 by hand: f = (j + 0.5) 3/7 - 0.5 = -2/7, 1/7, 4/7, 1, 10/7, 13/7, 16/7 clamped to [0, 2]
    i0, i1, t = upsample_plan(3, 7)
    assert i0.tolist() == [0, 0, 0, 1, 1, 1, 2] and i1.tolist() == [1, 1, 1, 2, 2, 2, 2]
    assert np.allclose(t, [0, 1 / 7, 4 / 7, 0, 3 / 7, 6 / 7, 0], atol=1e-7)
    with pytest.raises(ValueError):
        upsample_plan(0, 4)
    with pytest.raises(ValueError):
        upsample_plan(4, 0)


def test_default_lut_is_an_integer_ramp():
    from soft_contrastive_learning_amd.evaluation.saliency import default_lut
    lut = default_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert lut[0].tolist() == [0, 0, 255] and lut[85].tolist() == [0, 255, 255]
    assert lut[170].tolist() == [255, 255, 0] and lut[255].tolist() == [255, 0, 0]
    assert lut[1].tolist() == [0, 3, 255] and lut[86].tolist() == [3, 255, 252] and lut[254].tolist() == [255, 3, 0]
    step = np.abs(np.diff(lut.astype(int), axis=0)).sum(1)
    assert set(step.tolist()) <= {3, 6}                                 # no jump anywhere along the ramp


# ---- saliency_map_np --------------------------------------------------------------------------------

def test_saliency_map_np_on_constructed_cases():
    from soft_contrastive_learning_amd.evaluation.saliency import saliency_map_np
    b, h, w, c = 2, 3, 4, 512
    rng = np.random.default_rng(0)
    # one active channel: the map is that channel's activation times its mean gradient
    act = np.zeros((b, h, w, c), np.float32)
    grad = np.zeros((b, h, w, c), np.float32)
    act[..., 17] = rng.uniform(0.5, 2.0, (b, h, w))
    grad[..., 17] = rng.uniform(0.1, 1.0, (b, h, w))
    m, top = saliency_map_np(act, grad, 'gradcam')
    want = act[..., 17].astype(np.float64) * grad[..., 17].astype(np.float64).mean((1, 2))[:, None, None]
    assert m.dtype == np.float64 and m.shape == (b, h, w) and np.allclose(m, want, rtol=1e-14)
    assert np.array_equal(top, m.reshape(b, -1).max(1))
    # negative evidence -> 0
    m, top = saliency_map_np(act, -grad, 'gradcam')
    assert (m == 0).all() and (top == 0).all()
    # channels that cancel in the mean carry no weight
    grad2 = grad.copy()
    grad2[..., 40] = np.where(np.arange(h * w).reshape(h, w) % 2 == 0, 1.0, -1.0)
    act2 = act.copy()
    act2[..., 40] = 5.0
    assert np.allclose(saliency_map_np(act2, grad2, 'gradcam')[0], want, rtol=1e-14)
    # GRADNORM of a one-hot gradient: 1 at that position, 0 elsewhere; the activation is not read
    onehot = np.zeros((b, h, w, c), np.float32)
    onehot[0, 1, 2, 300] = 1.0
    onehot[1, 2, 0, 5] = -1.0
    m, top = saliency_map_np(None, onehot, 'gradnorm')
    want = np.zeros((b, h, w))
    want[0, 1, 2] = want[1, 2, 0] = 1.0
    assert np.array_equal(m, want) and top.tolist() == [1.0, 1.0]
    m, _ = saliency_map_np(None, 3.0 * onehot + 4.0 * np.roll(onehot, 1, axis=3), 'gradnorm')
    assert m[0, 1, 2] == 5.0
    with pytest.raises(ValueError):
        saliency_map_np(act, grad, 'gradxact')
    with pytest.raises(ValueError):
        saliency_map_np(act[:, :2], grad, 'gradcam')


# ---- overlay_np -------------------------------------------------------------------------------------

def test_overlay_np_on_constructed_cases():
    from soft_contrastive_learning_amd.evaluation.saliency import default_lut, overlay_np
    rng = np.random.default_rng(1)
    b, h, w, H, W = 2, 3, 5, 12, 17
    m = rng.uniform(0, 2, (b, h, w)).astype(np.float32)
    scale = m.reshape(b, -1).max(1)
    frame = rng.integers(0, 256, (b, H, W, 3), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    # alpha = 0: the frame exactly ((256 f + 128) >> 8 = f)
    assert np.array_equal(overlay_np(m, scale, frame, lut, 0), frame)
    # alpha = 256: lut[q], whatever the frame; a constant map at the scale is q = 255, at half 128
    full = overlay_np(m, scale, frame, lut, 256)
    assert np.array_equal(full, overlay_np(m, scale, 255 - frame, lut, 256))
    ones = np.ones((b, h, w), np.float32)
    assert (overlay_np(ones, [1.0, 1.0], frame, lut, 256) == lut[255]).all()
    assert (overlay_np(ones, [2.0, 2.0], frame, lut, 256) == lut[128]).all()         # (int)(127.5 + 0.5)
    assert (overlay_np(ones, [0.5, 0.25], frame, lut, 256) == lut[255]).all()         # clamped at 1
    assert (overlay_np(-ones, [1.0, 1.0], frame, lut, 256) == lut[0]).all()           # and at 0
    # the map's own pixels where the sizes agree: q = (int)(m / scale 255 + 0.5)
    same = overlay_np(m, scale, frame[:, :h, :w], lut, 256)
    q = (m / scale[:, None, None] * np.float32(255) + np.float32(0.5)).astype(np.int32)
    assert np.array_equal(same, lut[q])
    # scale = 0 (also negative, NaN): q = 0 everywhere
    for s in (0.0, -1.0, np.nan):
        got = overlay_np(m, [s, scale[1]], frame, lut, 256)
        assert (got[0] == lut[0]).all() and np.array_equal(got[1], full[1])
    # one NaN entry: index 0 where it reaches (the 2 x 2 samples that read it), nothing else moves
    bad = m.copy()
    bad[0, 1, 2] = np.nan
    lut0 = lut.copy()
    lut0[0] = [1, 2, 3]
    lut0[1:] = np.maximum(lut0[1:], 4)
    got, ref = overlay_np(bad, scale, frame, lut0, 256), overlay_np(m, scale, frame, lut0, 256)
    from soft_contrastive_learning_amd.evaluation.saliency import upsample_plan
    y0, y1, _ = upsample_plan(h, H)
    x0, x1, _ = upsample_plan(w, W)
    reach = ((y0 == 1) | (y1 == 1))[:, None] & ((x0 == 2) | (x1 == 2))[None, :]
    assert reach.any() and (got[0][reach] == [1, 2, 3]).all()
    assert np.array_equal(got[0][~reach], ref[0][~reach]) and np.array_equal(got[1], ref[1])
    # the blend: (alpha lut + (256 - alpha) frame + 128) >> 8, per channel
    mid = overlay_np(m, scale, frame, lut, 77)
    want = (77 * full.astype(np.int32) + 179 * frame.astype(np.int32) + 128) >> 8
    assert mid.dtype == np.uint8 and np.array_equal(mid, want)
    assert overlay_np(m, scale, frame, default_lut(), 128).shape == (b, H, W, 3)
    with pytest.raises(ValueError):
        overlay_np(m, scale, frame, lut, 257)


def test_alpha_is_rounded_to_the_integer_the_kernel_takes():
    from soft_contrastive_learning_amd.evaluation.saliency import alpha_int
    assert [alpha_int(a) for a in (0, 0.3, 0.5, 1.0)] == [0, 77, 128, 256]
    with pytest.raises(ValueError):
        alpha_int(1.01)
    with pytest.raises(ValueError):
        alpha_int(-0.01)


# ---- the C ABI --------------------------------------------------------------------------------------

def test_signatures_hold_both_names(lib):
    from soft_contrastive_learning_amd import _lib
    diag = _lib.load(diag=True)
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None and getattr(diag, name) is not None
    assert len(_lib.SIGNATURES['scl_saliency_map'][1]) == 10
    assert len(_lib.SIGNATURES['scl_saliency_overlay'][1]) == 18
    assert lib.scl_abi_version() == 12


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    from soft_contrastive_learning_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, a8, a2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 2)
    cam, norm = _lib.SALIENCY_GRADCAM, _lib.SALIENCY_GRADNORM

    def smap(act=p, grad=p, dtype=0, b=2, h=3, w=5, mode=cam, out=p, top=p):
        return lib.scl_saliency_map(act, grad, dtype, b, h, w, mode, out, top, None)

    # NULL operands — before the shape
    for kw in (dict(act=None), dict(grad=None), dict(out=None), dict(top=None)):
        assert smap(b=0, **kw) == NULL, kw
    assert smap(act=None, mode=norm, b=0) == SHAPE            # the gradient norm does not read act
    # empty and absurd shapes, misaligned operands — before the selectors
    for kw in (dict(b=0), dict(h=0), dict(w=0), dict(b=-1), dict(h=-3), dict(b=65536), dict(h=16385), dict(w=16385),
               dict(h=4096, w=4096), dict(act=a8), dict(grad=a8), dict(out=a2), dict(top=a2)):
        assert smap(dtype=7, **kw) == SHAPE, kw
    assert smap(dtype=7, b=0) == SHAPE
    assert smap(dtype=2) == KIND and smap(dtype=-1) == KIND and smap(mode=2) == KIND and smap(mode=-1) == KIND

    def over(b=2, h=3, w=5, H=12, W=17, alpha=128, **kw):
        a = dict(map=p, scale=p, frame=p, y0=p, y1=p, ty=p, x0=p, x1=p, tx=p, lut=p, out=p)
        a.update(kw)
        return lib.scl_saliency_overlay(a['map'], a['scale'], b, h, w, a['frame'], H, W, a['y0'], a['y1'], a['ty'],
                                        a['x0'], a['x1'], a['tx'], a['lut'], alpha, a['out'], None)

    for name in ('map', 'scale', 'frame', 'y0', 'y1', 'ty', 'x0', 'x1', 'tx', 'lut', 'out'):
        assert over(b=0, **{name: None}) == NULL, name
    for kw in (dict(b=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(b=-2), dict(H=-1), dict(b=65536),
               dict(h=16385), dict(W=16385), dict(H=16385), dict(h=4096, w=4096), dict(b=65535, H=16384, W=16384),
               dict(alpha=-1), dict(alpha=257), dict(map=a2), dict(scale=a2), dict(ty=a2), dict(x0=a2)):
        assert over(**kw) == SHAPE, kw

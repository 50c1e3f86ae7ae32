"""Match saliency: which parts of a frame made it match a place.

The localiser (``evaluation/localize.py``) says where a frame matched; when the top hit is a
look-alike place two kilometres away, the first thing one wants is a picture of what the network
looked at.  The reference carries ``model/grad_nets.py`` for that: the network with the conv5_3 map
(``grad_in``) exposed, so that a gradient can be taken there.  This module takes it and draws it:

* ``MatchSaliency.explain(images, target)``: one forward pass, the score
  ``s_b = -|out_b - target_b|^2`` (a similarity: positive evidence speaks FOR the match), its gradient
  at the map through the head alone — the backbone never runs backward — and the reduction of
  (activation, gradient) to one number per map position (``scl_saliency_map``, csrc/saliency.hip);
* ``overlay(frames, map, scale)``: the map stretched bilinearly over the frames, through a colour
  table, blended in (``scl_saliency_overlay``);
* ``Localizer.explain`` (evaluation/localize.py) explains a frame against its own k-th hit; the
  command below explains one image against another.

**Definitions** (``saliency_map_np`` / ``overlay_np`` / ``upsample_plan`` are their executable
statement; the kernels are tested against them).  With P = h w positions and C = 512 channels:

* ``'gradcam'``: ``w[b,c] = mean_p grad[b,p,c]``, ``map[b,p] = max(0, sum_c w[b,c] act[b,p,c])``
  (Selvaraju et al., Grad-CAM, ICCV 2017, at the conv5_3 map);
* ``'gradnorm'``: ``map[b,p] = sqrt(sum_c grad[b,p,c]^2)``: how strongly the score reacts to the
  position, without a sign.

A "gradient x activation" mode is deliberately not offered: with the channel L2 norm in front of the
head, the descriptor does not change when one position's vector is scaled, so
``sum_c grad[p,c] act[p,c]`` is zero at every position up to rounding.

Command::

    python -m soft_contrastive_learning_amd.evaluation.saliency --checkpoint STEM --query_img Q \\
        --ref_img R --out O.png [--pca_lv_pickle P --D 256] [--mode gradcam|gradnorm] [--alpha 0.5] \\
        [--rule resize_img|standard_size|none] [--dtype f32|bf16] [--vlad_cores 64|0] \\
        [--reduction none|1fc|2fc|3fc --out_dim 512]
"""
import numpy as np
import torch

from .. import _lib as L

MODES = {'gradcam': L.SALIENCY_GRADCAM, 'gradnorm': L.SALIENCY_GRADNORM}
_F32 = np.float32


def _mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    return MODES[mode]


# ---- the NumPy statement of the contract ----------------------------------------------------------

def upsample_plan(src, dst):
    """Axis tables of the bilinear stretch of ``src`` samples over ``dst`` (half-pixel centres, clamped
    at the border: ``F.interpolate(mode='bilinear', align_corners=False)``'s geometry) ->
    (i0 int32 [dst], i1 int32 [dst], t float32 [dst]): destination j reads
    ``m[i0] + (m[i1] - m[i0]) t``.  Computed in float64; they depend on the sizes alone."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError('upsample_plan: sizes must be at least 1, got %d -> %d' % (src, dst))
    f = (np.arange(dst, dtype=np.float64) + 0.5) * src / dst - 0.5
    f = np.clip(f, 0.0, src - 1.0)
    i0 = np.floor(f)
    i1 = np.minimum(i0 + 1, src - 1)
    return i0.astype(np.int32), i1.astype(np.int32), (f - i0).astype(np.float32)


def default_lut():
    """uint8 [256, 3]: blue -> cyan -> yellow -> red in three ramps of 85 steps of 3, integers only."""
    i = np.arange(256)
    seg = np.minimum(i // 85, 2)
    up = 3 * (i - 85 * seg)                      # 0 .. 255 along the segment
    zero, full = np.zeros_like(i), np.full_like(i, 255)
    r = np.choose(seg, [zero, up, full])
    g = np.choose(seg, [up, full, 255 - up])
    b = np.choose(seg, [full, 255 - up, zero])
    return np.stack([r, g, b], axis=1).astype(np.uint8)


def saliency_map_np(act, grad, mode='gradcam'):
    """The definition of ``saliency_map`` in float64: act, grad [B, h, w, C] -> (map [B, h, w],
    max [B]).  (``max(0, .)`` keeps a NaN, like the kernel; the maximum there skips it.)"""
    mode = _mode(mode)
    g = np.asarray(grad, dtype=np.float64)
    b, h, w, c = g.shape
    if mode == L.SALIENCY_GRADNORM:
        out = np.sqrt((g * g).sum(-1))
    else:
        a = np.asarray(act, dtype=np.float64)
        if a.shape != g.shape:
            raise ValueError('act %s and grad %s differ in shape' % (a.shape, g.shape))
        weight = g.reshape(b, h * w, c).sum(1) * (1.0 / (h * w))
        out = np.maximum(0.0, np.einsum('bc,bhwc->bhw', weight, a))
    return out, out.reshape(b, -1).max(1)


def overlay_np(map, scale, frame, lut, alpha):
    """The definition of ``overlay`` in NumPy: float32, one NumPy operation per operation of the
    kernel.  map [B, h, w] float32, scale [B], frame uint8 [B, H, W, 3], lut uint8 [256, 3],
    ``alpha`` the integer 0 .. 256 -> uint8 [B, H, W, 3]."""
    m = np.asarray(map, dtype=_F32)
    s = np.asarray(scale, dtype=_F32).reshape(-1, 1, 1)
    frame = np.asarray(frame, dtype=np.uint8)
    lut = np.asarray(lut, dtype=np.uint8)
    alpha = int(alpha)
    if not 0 <= alpha <= 256:
        raise ValueError('alpha must be an integer in 0 .. 256, got %r' % (alpha,))
    _, h, w = m.shape
    _, H, W, _ = frame.shape
    y0, y1, ty = upsample_plan(h, H)
    x0, x1, tx = upsample_plan(w, W)
    ty = ty[None, :, None]
    tx = tx[None, None, :]
    with np.errstate(all='ignore'):
        r0, r1 = m[:, y0], m[:, y1]                                   # [B, H, w]
        top = r0[:, :, x0] + (r0[:, :, x1] - r0[:, :, x0]) * tx
        bot = r1[:, :, x0] + (r1[:, :, x1] - r1[:, :, x0]) * tx
        v = top + (bot - top) * ty
        r = np.where(s > 0, v / s, _F32(0))
        r = np.where(r == r, np.minimum(np.maximum(r, _F32(0)), _F32(1)), _F32(0)).astype(_F32)
        q = (r * _F32(255) + _F32(0.5)).astype(np.int32)
    colour = lut[q].astype(np.int32)                                  # [B, H, W, 3]
    return ((alpha * colour + (256 - alpha) * frame.astype(np.int32) + 128) >> 8).astype(np.uint8)


# ---- the device calls -----------------------------------------------------------------------------

def saliency_map(act, grad, mode='gradcam'):
    """act, grad [B, h, w, 512] device tensors, float32 or bf16 (``act`` may be None for
    ``'gradnorm'``) -> (map [B, h, w] float32, max [B] float32) on the current stream."""
    mode = _mode(mode)
    L.require_device(act, grad)
    if grad.dim() != 4 or grad.shape[3] != L.VLAD_D:
        raise ValueError('grad must be [B, h, w, 512] channels-last, got %s' % (tuple(grad.shape),))
    if grad.dtype == torch.float32:
        dt = L.DT_F32
    elif grad.dtype == torch.bfloat16:
        dt = L.DT_BF16
    else:
        raise ValueError('the map must be float32 or bfloat16, got %s' % grad.dtype)
    if act is not None and (act.shape != grad.shape or act.dtype != grad.dtype or act.device != grad.device):
        raise ValueError('act %s %s and grad %s %s must agree in shape, dtype and device'
                         % (tuple(act.shape), act.dtype, tuple(grad.shape), grad.dtype))
    if act is None and mode == L.SALIENCY_GRADCAM:
        raise ValueError("'gradcam' needs the activation")
    grad = grad.detach().contiguous()
    act = None if act is None else act.detach().contiguous()
    b, h, w, _ = grad.shape
    out = torch.empty((b, h, w), dtype=torch.float32, device=grad.device)
    top = torch.empty(b, dtype=torch.float32, device=grad.device)
    with torch.cuda.device(grad.device):
        L.check(L.load().scl_saliency_map(L.ptr(act), L.ptr(grad), dt, b, h, w, mode, L.ptr(out), L.ptr(top),
                                          L.stream_of(grad)))
    return out, top


_PLANS = {}        # (h, w, H, W, device) -> the six axis tables on the device
_LUTS = {}         # device -> default_lut() there


def _device_plan(h, w, H, W, dev):
    key = (h, w, H, W, dev)
    tabs = _PLANS.get(key)
    if tabs is None:
        if len(_PLANS) >= 64:
            _PLANS.clear()
        tabs = _PLANS[key] = tuple(torch.from_numpy(t).to(dev) for t in upsample_plan(h, H) + upsample_plan(w, W))
    return tabs


def alpha_int(alpha):
    """The blend weight as the integer the kernel takes: ``round(256 alpha)``."""
    a = int(round(256.0 * float(alpha)))
    if not 0 <= a <= 256:
        raise ValueError('alpha must lie in [0, 1], got %r' % (alpha,))
    return a


def overlay(frames_u8, map, scale, alpha=0.5, lut=None):
    """frames_u8 uint8 [B, H, W, 3] (device tensor, or NumPy: uploaded to the map's device), map
    [B, h, w] float32 and scale [B] float32 device tensors (``explain``'s results), ``alpha`` the
    weight of the colours in [0, 1], ``lut`` uint8 [256, 3] (None: ``default_lut()``) ->
    uint8 [B, H, W, 3] on the device, on the current stream.  The axis tables are cached per
    (h, w, H, W)."""
    L.require_device(map, scale)
    dev = map.device
    frames = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError('frames must be uint8 [B, H, W, 3], got %s %s' % (frames.dtype, tuple(frames.shape)))
    frames = frames.to(dev).contiguous()
    if map.dim() != 3 or map.shape[0] != frames.shape[0] or tuple(scale.shape) != (frames.shape[0],):
        raise ValueError('map %s and scale %s must be [B, h, w] and [B] for B = %d frames'
                         % (tuple(map.shape), tuple(scale.shape), frames.shape[0]))
    if lut is None:
        table = _LUTS.get(dev)
        if table is None:
            table = _LUTS[dev] = torch.from_numpy(default_lut()).to(dev)
    else:
        table = lut if isinstance(lut, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lut))
        if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
            raise ValueError('lut must be uint8 [256, 3], got %s %s' % (table.dtype, tuple(table.shape)))
        table = table.to(dev).contiguous()
    m = map.detach().to(torch.float32).contiguous()
    s = scale.detach().to(torch.float32).contiguous()
    b, H, W, _ = frames.shape
    _, h, w = m.shape
    y0, y1, ty, x0, x1, tx = _device_plan(h, w, H, W, dev)
    out = torch.empty_like(frames)
    with torch.cuda.device(dev):
        L.check(L.load().scl_saliency_overlay(L.ptr(m), L.ptr(s), b, h, w, L.ptr(frames), H, W, L.ptr(y0),
                                              L.ptr(y1), L.ptr(ty), L.ptr(x0), L.ptr(x1), L.ptr(tx),
                                              L.ptr(table), alpha_int(alpha), L.ptr(out), L.stream_of(m)))
    return out


class MatchSaliency:
    """``MatchSaliency(model=None, pca=None)``: ``model`` the network (None:
    ``nets.default_model()``), ``pca`` a fitted ``PCAWhitening`` when the targets live in the whitened
    space the localiser compares in."""

    def __init__(self, model=None, pca=None):
        self.model = model
        self.pca = pca

    def _model(self):
        from ..model import nets
        return self.model or nets.default_model()

    def _batch(self, images):
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        return t.to(next(self._model().parameters()).device)

    def _output(self, first):
        """``nets.output``'s tail on the first value of grad_nets' forward, then the whitening as
        differentiable float32 operations."""
        model = self._model()
        out = first if getattr(model, 'vlad_cores', 64) == 64 else first.reshape(first.shape[0], -1)
        head = getattr(model, 'reduction_head', None)
        out = (out if head is None else head(out)).float()
        if self.pca is not None:
            if getattr(self.pca, '_proj', None) is None:
                raise RuntimeError('MatchSaliency needs a fitted PCAWhitening (its projection is '
                                   'differentiated through)')
            out = out @ self.pca._proj.to(out.device) - self.pca._offset.to(out.device)
        return out

    def _forward(self, images):
        """(out [B, D], grad_in): grad_nets' forward, cut at the map — the backbone under ``no_grad``,
        the head recorded — and ``_output``.  Call it under ``enable_grad``.

        Everything above the map repeats its bits from call to call; the backbone does where its
        layers run on the package's own kernels.  Layers that go to the library convolutions
        (float32 models, small maps) need not: measured at 32 x 48, two passes over one input differ
        by 2e-4 on the float32 map and by two bf16 steps on the bf16 one.  (torch's deterministic
        switch is no way out: the library then refuses some of these layers when they have not run
        before, and took 165 ms for one 180 x 240 frame.)"""
        from ..model import grad_nets
        model = self._model()
        fn = grad_nets.vgg16Netvlad if getattr(model, 'vlad_cores', 64) == 64 else grad_nets.vgg16
        first, grad_in = fn(self._batch(images), model=model, cut=True)
        return self._output(first), grad_in

    def embed(self, images):
        """images [B, H, W, {1|3}] raw 0..255 -> [B, D] in the space ``explain`` compares in, detached.
        The same calls as ``explain``'s own forward pass (the head's kernels in a recorded pass need
        not be the ones of an inference pass), so a frame is at distance exactly 0 from itself
        wherever the backbone repeats its bits (``_forward``); elsewhere at rounding distance, and
        its map is rounding noise of the order 1e-9 that ``overlay`` would stretch to full contrast."""
        with torch.enable_grad():
            return self._forward(images)[0].detach()

    def map_gradient(self, images, target):
        """(grad_in, gradient of ``sum_b -|out_b - target_b|^2`` at it, squared distances [B]): one
        forward pass and one backward pass of the head.  The backbone runs under ``no_grad`` and the
        graph is cut at the map; parameters receive no gradients."""
        from ..model import nets
        sink, nets.GRAD_SINK = nets.GRAD_SINK, None        # a trainer's gradient buffer is not ours to write
        try:
            with torch.enable_grad():
                out, grad_in = self._forward(images)
                tgt = target if isinstance(target, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(target))
                tgt = tgt.detach().to(out.device, torch.float32)
                if tuple(tgt.shape) != tuple(out.shape):
                    raise ValueError('target %s must be %s, the space the model (and the whitening) puts '
                                     'the frames in' % (tuple(tgt.shape), tuple(out.shape)))
                d2 = ((out - tgt) ** 2).sum(dim=1)
                (g,) = torch.autograd.grad(-d2.sum(), grad_in)
        finally:
            nets.GRAD_SINK = sink
        return grad_in.detach(), g, d2.detach()

    def explain(self, images, target, mode='gradcam'):
        """images [B, H, W, {1|3}] raw 0..255, target [B, D] -> (map [B, h, w] float32, scale [B]
        float32: the map's maximum per frame) on the device."""
        _mode(mode)
        act, g, _ = self.map_gradient(images, target)
        return saliency_map(act, g, mode)

    def explain_pair(self, query_images, ref_images, mode='gradcam'):
        """``explain`` of the query frames against the same model's output for ``ref_images``."""
        return self.explain(query_images, self.embed(ref_images), mode)


# ---- the command ----------------------------------------------------------------------------------

def main_parser():
    import argparse
    from ..model import reduction
    p = argparse.ArgumentParser()
    p.add_argument('--checkpoint', default='', help='checkpoint stem (empty: the initialised model)')
    p.add_argument('--query_img', required=True)
    p.add_argument('--ref_img', required=True)
    p.add_argument('--out', required=True, help='the overlay on the sized query frame (PNG)')
    p.add_argument('--pca_lv_pickle', default='', help='descriptors to fit the whitening on (with --D)')
    p.add_argument('--D', default=256, type=int, help='PCA dimension (used with --pca_lv_pickle)')
    p.add_argument('--mode', default='gradcam', choices=sorted(MODES))
    p.add_argument('--alpha', default=0.5, type=float)
    p.add_argument('--rule', default='resize_img', choices=['resize_img', 'standard_size', 'none'])
    p.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    p.add_argument('--vlad_cores', default=64, type=int, choices=[64, 0])
    p.add_argument('--reduction', default='none', choices=('none',) + tuple(reduction.KINDS))
    p.add_argument('--out_dim', default=512, type=int)
    return p


def main(argv=None):
    """Explains ``--query_img`` against ``--ref_img``: both are loaded (``util.io.load_img``), sized by
    the loaders' rule, the pair is explained and the overlay on the sized query frame is written
    (``util.io.save_img``).  Prints the feature distance and the map's maximum; returns them."""
    from .. import checkpoint
    from ..model import nets, reduction
    from ..util import io
    from .inference import size_on_host
    from .pca import PCAWhitening
    flags = main_parser().parse_args(argv)
    dtype = torch.float32 if flags.dtype == 'f32' else torch.bfloat16
    model = nets.VGG16NetVLAD(compute_dtype=dtype, vlad_cores=flags.vlad_cores).cuda()
    if flags.reduction != 'none':
        reduction.attach(model, flags.reduction, flags.out_dim)
    if flags.checkpoint:
        checkpoint.load(model, flags.checkpoint)
    pca = None
    if flags.pca_lv_pickle:
        pca = PCAWhitening(flags.D, device='cuda').fit(np.array(io.load_pickle(flags.pca_lv_pickle), dtype=np.float32))
    kw = {'resize_img': dict(max_size=240), 'standard_size': dict(h=180, w=240), 'none': {}}[flags.rule]
    query = np.asarray(size_on_host(io.load_img(flags.query_img), flags.rule, kw), dtype=np.uint8)
    ref = np.asarray(size_on_host(io.load_img(flags.ref_img), flags.rule, kw), dtype=np.uint8)
    sal = MatchSaliency(model, pca)
    target = sal.embed(ref[None].astype(np.float32))
    act, g, d2 = sal.map_gradient(query[None].astype(np.float32), target)
    m, top = saliency_map(act, g, flags.mode)
    io.save_img(overlay(query[None], m, top, flags.alpha)[0].cpu().numpy(), flags.out)
    dist, peak = float(d2[0].sqrt()), float(top[0])
    print('feature distance {:.6g}, map maximum {:.6g} ({}), wrote {}'.format(dist, peak, flags.mode, flags.out))
    return dist, peak


if __name__ == '__main__':
    main()

"""The loaders' resize on the device: ``util/cv.py``'s 8-bit bilinear resampler applied by a HIP
kernel (csrc/frames.hip ``scl_frames_resize``) to frames as the camera or the decoder delivers them.

The host computes the plan (``cv.resize_plan``: four small int32 tables per axis, the whole of the
float32 coordinate arithmetic), the device only applies it in int32 — so the device pixels ARE the
host pixels, and descriptors, whitening and certified lists downstream see the same bits.  The
tables of a plan are uploaded once per (source size, rule, parameters) and stay on the device: a
steady stream of same-sized frames uploads frames only.

There is no CPU fallback: ``util/cv.py`` is the host resampler, this module needs a HIP device.
"""
import numpy as np
import torch

from .. import _lib
from . import cv

_OUT_KINDS = {torch.uint8: _lib.FRAMES_U8, torch.float32: _lib.FRAMES_F32}


def apply_tables(src, xtab, ytab, out):
    """One ``scl_frames_resize`` launch on the current stream: ``src`` uint8 [n,sh,sw,c] (dense,
    any byte address), ``xtab`` int32 [4,ow] and ``ytab`` int32 [4,oh] on the device (``ResizePlan
    .xtab() / .ytab()``), ``out`` [n,oh,ow,c] uint8 or float32 (dense).  Returns ``out``."""
    from ..model import nets
    _lib.require_device(src, xtab, ytab, out)
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_contiguous():
        raise ValueError('apply_tables: src is a dense uint8 [n,sh,sw,c]')
    if out.dtype not in _OUT_KINDS or not out.is_contiguous():
        raise ValueError('apply_tables: out is a dense uint8 or float32 tensor')
    for t in (xtab, ytab):
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != 4 or not t.is_contiguous():
            raise ValueError('apply_tables: a table is a dense int32 [4, length]')
    n, sh, sw, c = src.shape
    oh, ow = int(ytab.shape[1]), int(xtab.shape[1])
    if tuple(out.shape) != (n, oh, ow, c):
        raise ValueError('apply_tables: out is %s, the tables make %s'
                         % (tuple(out.shape), (n, oh, ow, c)))
    _lib.check(_lib.load().scl_frames_resize(
        _lib.ptr(src), n, sh, sw, c, _lib.ptr(xtab), ow, _lib.ptr(ytab), oh, _OUT_KINDS[out.dtype],
        _lib.ptr(out), _lib.stream_of(out)))
    nets._work('frames_resize_kernel', 0.0, kernel_bytes(n, oh, ow, c, out.element_size()))
    return out


def kernel_bytes(n, oh, ow, c, out_itemsize):
    """The bytes one launch needs, from its shapes: per output value 2 x 2 source bytes in and one
    value out, per output row and column 16 table bytes."""
    return float(n) * oh * ow * c * (4 + out_itemsize) + 16.0 * (oh + ow)


def debayer_tables(raw, pattern, border, lut, xtab, ytab, out):
    """One ``scl_frames_debayer`` launch on the current stream: ``raw`` uint8 [n,sh,sw] (dense, any
    byte address), ``pattern`` / ``border`` names of ``_lib.BAYER_PATTERNS`` / ``_lib.BAYER_BORDERS``,
    ``lut`` float64 [2,sh*sw] on the device or None (demosaic only), ``xtab`` / ``ytab`` as for
    ``apply_tables`` or both None (full size), ``out`` [n,oh,ow,3] uint8 or float32.  Returns ``out``."""
    from ..model import nets
    _lib.require_device(raw, lut, xtab, ytab, out)
    if raw.dtype != torch.uint8 or raw.dim() != 3 or not raw.is_contiguous():
        raise ValueError('debayer_tables: raw is a dense uint8 [n,sh,sw]')
    if out.dtype not in _OUT_KINDS or not out.is_contiguous():
        raise ValueError('debayer_tables: out is a dense uint8 or float32 tensor')
    if pattern not in _lib.BAYER_PATTERNS or border not in _lib.BAYER_BORDERS:
        raise ValueError('debayer_tables: pattern is one of %s and border one of %s, not %r, %r'
                         % (_lib.BAYER_PATTERNS, _lib.BAYER_BORDERS, pattern, border))
    n, sh, sw = raw.shape
    if lut is not None and (lut.dtype != torch.float64 or tuple(lut.shape) != (2, sh * sw)
                            or not lut.is_contiguous()):
        raise ValueError('Incorrect image size for camera model: lut is a dense float64 [2, %d] for '
                         'frames of %d x %d, not %s %s' % (sh * sw, sw, sh, lut.dtype, tuple(lut.shape)))
    if (xtab is None) != (ytab is None):
        raise ValueError('debayer_tables: both tables or none')
    oh, ow = sh, sw
    if xtab is not None:
        for t in (xtab, ytab):
            if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != 4 or not t.is_contiguous():
                raise ValueError('debayer_tables: a table is a dense int32 [4, length]')
        oh, ow = int(ytab.shape[1]), int(xtab.shape[1])
    if tuple(out.shape) != (n, oh, ow, 3):
        raise ValueError('debayer_tables: out is %s, the frames and tables make %s'
                         % (tuple(out.shape), (n, oh, ow, 3)))
    _lib.check(_lib.load().scl_frames_debayer(
        _lib.ptr(raw), n, sh, sw, _lib.BAYER_PATTERNS.index(pattern), _lib.BAYER_BORDERS.index(border),
        _lib.ptr(lut), _lib.ptr(xtab), ow, _lib.ptr(ytab), oh, _OUT_KINDS[out.dtype], _lib.ptr(out),
        _lib.stream_of(out)))
    nets._work('frames_debayer_kernel', 0.0,
               debayer_bytes(n, sh, sw, oh, ow, out.element_size(), lut is not None, xtab is not None))
    return out


def debayer_bytes(n, sh, sw, oh, ow, out_itemsize, lut=True, fused=False):
    """The bytes one launch needs, from its shapes: per evaluated pixel (every pixel of the frame at
    full size, four per output pixel with tables) 16 table bytes once and a 4 x 4 raw window per
    frame; three values out per output pixel and frame; the resize tables."""
    evaluated = 4.0 * oh * ow if fused else float(sh) * sw
    return (evaluated * (16.0 * bool(lut) + 16.0 * n) + 3.0 * n * oh * ow * out_itemsize
            + (16.0 * (oh + ow) if fused else 0.0))


class DeviceResizer:
    """``DeviceResizer(device)``: ``resize_img`` / ``standard_size`` / ``resize_linear`` of
    ``util/cv.py`` for uint8 frames — a NumPy array or a tensor (host or device), ``[SH,SW,C]``,
    ``[n,SH,SW,C]``, ``[SH,SW]`` (grey) or a list of such frames of ONE shape, C = 1 or 3 — as a
    device tensor ``[n,oh,ow,C]`` (a single frame keeps a leading 1) on the caller's current stream.

    ``debayer`` takes raw one-channel Bayer frames through the RobotCar SDK's demosaic and
    undistortion first (``scl_frames_debayer``), fused with the same rules.

    The object owns the device copies of the plans' tables (``table_uploads`` counts them), of the
    distortion tables it was given (``lut_uploads``; one per table object, resident from then on) and a
    pinned staging buffer for host arrays, grown when a bigger batch arrives.  One resizer serves
    one thread at a time."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.SclError('DeviceResizer needs a HIP device (util/cv.py is the host resampler; '
                                'no CPU fallback exists); got %r' % (self.device,))
        self._tables = {}          # (sh, sw, rule, parameters) -> (xtab, ytab) on the device
        self._luts = {}            # (id, shape) of a distortion table -> (its device copy, the object)
        self.lut_uploads = 0
        self._staging = None       # pinned uint8 [capacity]
        self._staged = None        # event after the last copy out of the staging buffer
        self.table_uploads = 0

    # ---- frames ----------------------------------------------------------------------------
    @staticmethod
    def _as_batch(frames):
        """-> uint8 [n,SH,SW,C] (NumPy array or tensor, as given), or ValueError."""
        if isinstance(frames, (list, tuple)):
            if not frames:
                raise ValueError('DeviceResizer: no frames')
            if len({tuple(f.shape) for f in frames}) != 1:
                raise ValueError('DeviceResizer: the frames of one call share one shape; got %s'
                                 % sorted({tuple(f.shape) for f in frames}))
            if any(f.ndim not in (2, 3) for f in frames):
                raise ValueError('DeviceResizer: a frame is [SH,SW] or [SH,SW,C]')
            frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack(frames)
            if frames.ndim == 3:
                frames = frames[..., None]
        if not isinstance(frames, (np.ndarray, torch.Tensor)):
            raise ValueError('DeviceResizer takes a uint8 NumPy array or tensor, not %s' % type(frames).__name__)
        if frames.dtype != (torch.uint8 if isinstance(frames, torch.Tensor) else np.uint8):
            raise ValueError('DeviceResizer takes uint8 frames, not %s' % (frames.dtype,))
        if frames.ndim == 2:
            frames = frames[None, :, :, None]
        elif frames.ndim == 3:
            frames = frames[None]
        elif frames.ndim != 4:
            raise ValueError('DeviceResizer: frames are [SH,SW], [SH,SW,C] or [n,SH,SW,C], not %s'
                             % (tuple(frames.shape),))
        if frames.shape[3] not in (1, 3) or min(frames.shape) < 1:
            raise ValueError('DeviceResizer: %s is no batch of frames with 1 or 3 channels'
                             % (tuple(frames.shape),))
        return frames

    def _upload(self, frames):
        """uint8 [n,SH,SW,C] -> the same, dense, on the device (current stream)."""
        if isinstance(frames, torch.Tensor) and frames.is_cuda:
            if frames.device != self.device:
                raise ValueError('DeviceResizer(%s) was given frames on %s' % (self.device, frames.device))
            return frames.contiguous()
        host = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) \
            else frames.contiguous()
        dev = torch.empty(host.shape, dtype=torch.uint8, device=self.device)
        if host.is_pinned():
            return dev.copy_(host, non_blocking=True)
        nbytes = host.numel()
        if self._staged is not None:
            self._staged.synchronize()          # the previous batch has left the buffer
        if self._staging is None or self._staging.numel() < nbytes:
            self._staging = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        stage = self._staging[:nbytes].view(host.shape)
        stage.copy_(host)
        dev.copy_(stage, non_blocking=True)
        if self._staged is None:
            self._staged = torch.cuda.Event()
        self._staged.record(torch.cuda.current_stream(self.device))
        return dev

    # ---- plans -----------------------------------------------------------------------------
    def _device_tables(self, key, make_plan):
        hit = self._tables.get(key)
        if hit is None:
            plan = make_plan()
            both = np.concatenate([plan.xtab().ravel(), plan.ytab().ravel()])
            t = torch.from_numpy(both).to(self.device)
            # the tables serve every later call, under whatever stream it runs
            torch.cuda.current_stream(self.device).synchronize()
            hit = self._tables[key] = (t[:4 * plan.dw].view(4, plan.dw), t[4 * plan.dw:].view(4, plan.dh))
            self.table_uploads += 1
        return hit

    def _run(self, frames, rule, params, make_plan, out):
        if out not in _OUT_KINDS:
            raise ValueError('DeviceResizer: out is torch.uint8 or torch.float32, not %s' % (out,))
        batch = self._as_batch(frames)
        n, sh, sw, c = (int(v) for v in batch.shape)
        xtab, ytab = self._device_tables((sh, sw, rule) + params, lambda: make_plan(sh, sw))
        with torch.cuda.device(self.device):
            src = self._upload(batch)
            dst = torch.empty((n, ytab.shape[1], xtab.shape[1], c), dtype=out, device=self.device)
            return apply_tables(src, xtab, ytab, dst)

    # ---- the three rules of util/cv.py -----------------------------------------------------------
    def resize_img(self, frames, max_size=240, out=torch.float32):
        return self._run(frames, 'resize_img', (max_size,),
                         lambda sh, sw: cv.plan_resize_img(sh, sw, max_size), out)

    def standard_size(self, frames, h=180, w=240, out=torch.float32):
        return self._run(frames, 'standard_size', (h, w),
                         lambda sh, sw: cv.plan_standard_size(sh, sw, h, w), out)

    def apply(self, frames, rule='resize_img', out=torch.float32, **kw):
        """The loaders' sizing rules by name: ``'resize_img'`` (``max_size``), ``'standard_size'``
        (``h``, ``w``) or ``'none'`` (the frame as it is, only widened to ``out``)."""
        if rule == 'resize_img':
            return self.resize_img(frames, out=out, **kw)
        if rule == 'standard_size':
            return self.standard_size(frames, out=out, **kw)
        if rule == 'none' and not kw:
            return self.resize_linear(frames, fx=1.0, fy=1.0, out=out)     # weights 2048 : 0, exact
        raise ValueError("rule is 'resize_img', 'standard_size' or 'none' (no parameters), not %r %r"
                         % (rule, kw))

    # ---- raw Bayer frames (util/robotcar.py) -------------------------------------------------------
    @staticmethod
    def _as_raw_batch(frames):
        """-> uint8 [n,SH,SW] (NumPy array or tensor, as given), or ValueError."""
        if isinstance(frames, (list, tuple)):
            if not frames:
                raise ValueError('DeviceResizer: no frames')
            if len({tuple(f.shape) for f in frames}) != 1 or frames[0].ndim != 2:
                raise ValueError('DeviceResizer.debayer: the raw frames of one call are [SH,SW] of one shape; '
                                 'got %s' % sorted({tuple(f.shape) for f in frames}))
            frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack(frames)
        if not isinstance(frames, (np.ndarray, torch.Tensor)):
            raise ValueError('DeviceResizer takes a uint8 NumPy array or tensor, not %s' % type(frames).__name__)
        if frames.dtype != (torch.uint8 if isinstance(frames, torch.Tensor) else np.uint8):
            raise ValueError('DeviceResizer takes uint8 frames, not %s' % (frames.dtype,))
        if frames.ndim == 2:
            frames = frames[None]
        if frames.ndim != 3 or frames.shape[0] < 1 or min(frames.shape[1:]) < 2:
            raise ValueError('DeviceResizer.debayer: raw frames are one-channel, [SH,SW] or [n,SH,SW] with '
                             'both sides at least 2, not %s' % (tuple(frames.shape),))
        return frames

    def _device_lut(self, lut, sh, sw):
        """The table on the device, uploaded once per object (key: its ``id`` and shape; the object
        is kept, so the id stays its own)."""
        if lut is None:
            return None
        if not isinstance(lut, (np.ndarray, torch.Tensor)):
            raise ValueError('lut is a float64 NumPy array or tensor [2, SH*SW], not %s' % type(lut).__name__)
        if tuple(lut.shape) != (2, sh * sw) or lut.dtype not in (np.float64, torch.float64):
            raise ValueError('Incorrect image size for camera model: lut is %s %s, frames of %d x %d need '
                             'float64 [2, %d]' % (lut.dtype, tuple(lut.shape), sw, sh, sh * sw))
        key = (id(lut), tuple(lut.shape))
        hit = self._luts.get(key)
        if hit is None:
            host = torch.from_numpy(np.ascontiguousarray(lut)) if isinstance(lut, np.ndarray) else lut
            dev = host.to(self.device).contiguous()
            torch.cuda.current_stream(self.device).synchronize()      # serves every later stream
            hit = self._luts[key] = (dev, lut)
            self.lut_uploads += 1
        return hit[0]

    def _rule_tables(self, sh, sw, rule, kw):
        """The device tables of a sizing rule by name, from the cache ``resize_img`` /
        ``standard_size`` fill; (None, None) for 'none'."""
        if rule == 'none' and not kw:
            return None, None
        if rule == 'resize_img':
            def plan(max_size=240):
                return (max_size,), lambda: cv.plan_resize_img(sh, sw, max_size)
        elif rule == 'standard_size':
            def plan(h=180, w=240):
                return (h, w), lambda: cv.plan_standard_size(sh, sw, h, w)
        else:
            raise ValueError("rule is 'resize_img', 'standard_size' or 'none' (no parameters), not %r %r"
                             % (rule, kw))
        params, make = plan(**kw)
        return self._device_tables((sh, sw, rule) + params, make)

    def debayer(self, frames, pattern='gbrg', lut=None, border='reflect', rule='none', out=torch.uint8, **kw):
        """The RobotCar SDK's ``load_image`` of raw Bayer frames (``robotcar.load_image_np``: bilinear
        demosaic, undistortion by the camera's table ``lut`` — float64 [2,SH*SW], None: skipped —,
        byte), then the sizing rule ``rule`` / ``kw`` of ``apply`` on those bytes, in ONE launch: with
        a rule only the 2 x 2 undistorted pixels each output value reads are evaluated and the
        full-size RGB frame is never written.  ``frames``: uint8 [SH,SW], [n,SH,SW] or a list of one
        shape, host or device.  -> device [n,oh,ow,3] (``rule='none'``: [n,SH,SW,3])."""
        if out not in _OUT_KINDS:
            raise ValueError('DeviceResizer: out is torch.uint8 or torch.float32, not %s' % (out,))
        batch = self._as_raw_batch(frames)
        n, sh, sw = (int(v) for v in batch.shape)
        xtab, ytab = self._rule_tables(sh, sw, rule, kw)
        table = self._device_lut(lut, sh, sw)
        oh, ow = (sh, sw) if xtab is None else (int(ytab.shape[1]), int(xtab.shape[1]))
        with torch.cuda.device(self.device):
            src = self._upload(batch)
            dst = torch.empty((n, oh, ow, 3), dtype=out, device=self.device)
            return debayer_tables(src, pattern, border, table, xtab, ytab, dst)

    def resize_linear(self, frames, fx=None, fy=None, dsize=None, window=None, out=torch.uint8):
        """``window`` = (top, left, h, w) of the result, or None for all of it."""
        dsize = None if dsize is None else (int(dsize[0]), int(dsize[1]))
        window = None if window is None else tuple(int(v) for v in window)

        def make(sh, sw):
            plan = cv.resize_plan(sh, sw, fx, fy, dsize)
            return plan if window is None else plan.window(*window)
        return self._run(frames, 'resize_linear', (fx, fy, dsize, window), make, out)

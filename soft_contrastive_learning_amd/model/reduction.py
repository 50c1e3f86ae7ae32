"""Dense reduction heads of ``build_model`` (train/train.py:631-644; evaluation/inference.py:97-109).

``--reduction 1fc|2fc|3fc --out_dim D`` puts a stack of ``tf.layers.dense`` layers on
``ops['full_out']`` (the 32768-wide NetVLAD descriptor, or the flattened channel-normalised conv5_3
map with ``--vlad_cores 0``); their result is ``ops['output']``, which every consumer reads — the
loss, the hard-negative mining features and the localisation check:

    1fc   in -> D                                  fc1/{kernel,bias}
    2fc   in -> 4096 ReLU -> D                     dense/…, fc2/…
    3fc   in -> 4096 ReLU -> 4096 ReLU -> D        dense/…, dense_1/…, fc3/…

The layers are created outside the ``vgg16_netvlad_pca`` scope, so their names carry no prefix,
and the dropout layers named ``fc1`` / ``fc2`` create no variables.  The kernel is kept in TF's
layout [in, units] (y = x W + b), so checkpoints need no transpose.  ``tf.layers.dense``
initialises the kernel Glorot-uniform, limit sqrt(6 / (in + units)), and the bias with zeros.

TF 1.10 quirk: the reference calls ``tf.layers.dropout(fc1, ops['keep_prob'],
name='fc1')``.  The second positional argument of ``tf.layers.dropout`` is ``rate``, not
``keep_prob``, and ``training`` defaults to False, so the layer returns its input unchanged — also
in the training step, which feeds keep_prob 0.5 (train/train.py:273).  There is no dropout here.

On a HIP device every layer runs the float32 kernels of csrc/dense.hip (forward, backward-data,
weight / bias gradient; ``--dtype bf16`` too: the head is float32); on the CPU it is plain torch
float32 — the CPU composition the tests compare against.  Weight and bias gradients go straight
into the trainer's gradient buckets when ``nets.GRAD_SINK`` offers a view.
"""
import math

import torch

from .. import _lib
from . import nets

KINDS = ('1fc', '2fc', '3fc')
HIDDEN = 4096
MAX_ROWS = 256          # rows per library call (include/scl_hip.h)


def layer_specs(kind, in_dim, out_dim):
    """[(tf layer name, in, units, relu)] of a head kind."""
    if kind == '1fc':
        return [('fc1', in_dim, out_dim, False)]
    if kind == '2fc':
        return [('dense', in_dim, HIDDEN, True), ('fc2', HIDDEN, out_dim, False)]
    if kind == '3fc':
        return [('dense', in_dim, HIDDEN, True), ('dense_1', HIDDEN, HIDDEN, True),
                ('fc3', HIDDEN, out_dim, False)]
    raise ValueError('reduction %r is not a dense head (%s)' % (kind, ', '.join(KINDS)))


def head_in_dim(vlad_cores, height=180, width=240):
    """Static width of ``ops['full_out']``: 32768 with the NetVLAD head; without it the flattened
    conv5_3 map, H' W' 512 after VGG16's four floor-halving poolings (180 x 240 -> 11 x 15 x 512 =
    84480, the reference's fixed input, train/train.py:599-602)."""
    if vlad_cores == 64:
        return nets.L.VLAD_D * nets.L.VLAD_K
    h, w = int(height), int(width)
    for _ in range(4):
        h, w = h // 2, w // 2
    if h < 1 or w < 1:
        raise ValueError('image %d x %d has no conv5_3 map' % (height, width))
    return h * w * nets.L.VLAD_D


# ---- library calls (tensors on a HIP device, float32, unit stride along rows) -----------------------
def _rows(t):
    if t.dim() != 2 or t.stride(1) != 1:
        t = t.contiguous()
    return t


def dense_fwd(x, w, b, relu):
    """y = x w + b (ReLU): x [M,K], w [K,N] -> [M,N] (rows in calls of at most 256)."""
    _lib.require_device(x, w, b)
    x, w = _rows(x), _rows(w)
    M, K = x.shape
    N = w.shape[1]
    lib = _lib.load()
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(lib.scl_dense_fwd_workspace_bytes(min(M, MAX_ROWS), K, N), x.device)
    for r in range(0, M, MAX_ROWS):
        m = min(MAX_ROWS, M - r)
        _lib.check(lib.scl_dense_fwd(_lib.ptr(x[r:]), x.stride(0), _lib.ptr(w), w.stride(0),
                                     _lib.ptr(b), m, K, N, int(bool(relu)), _lib.ptr(y[r:]),
                                     y.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_of(x)))
    return y


def dense_bwd_data(gy, y, w):
    """gx = (gy masked by y > 0 when y is given) w^T -> [M,K]."""
    _lib.require_device(gy, y, w)
    gy, w = _rows(gy), _rows(w)
    y = None if y is None else _rows(y)
    M, N = gy.shape
    K = w.shape[0]
    lib = _lib.load()
    gx = torch.empty((M, K), dtype=torch.float32, device=gy.device)
    ws = _lib.workspace(lib.scl_dense_bwd_data_workspace_bytes(min(M, MAX_ROWS), K, N), gy.device)
    for r in range(0, M, MAX_ROWS):
        m = min(MAX_ROWS, M - r)
        _lib.check(lib.scl_dense_bwd_data(
            _lib.ptr(gy[r:]), gy.stride(0), None if y is None else _lib.ptr(y[r:]),
            0 if y is None else y.stride(0), _lib.ptr(w), w.stride(0), m, K, N, _lib.ptr(gx[r:]),
            gx.stride(0), _lib.ptr(ws), ws.numel(), _lib.stream_of(gy)))
    return gx


def dense_wgrad(x, gy, y, gw, gb):
    """gw = x^T gy', gb = sum_m gy' (gy' = gy masked by y > 0 when y is given), written into the
    given [K,N] / [N] tensors (gb may be None).  More than 256 rows: the 256-row results are added
    in row order."""
    _lib.require_device(x, gy, y, gw, gb)
    x, gy = _rows(x), _rows(gy)
    y = None if y is None else _rows(y)
    M, K = x.shape
    N = gy.shape[1]
    if gw.stride(1) != 1 or (gb is not None and not gb.is_contiguous()):
        raise ValueError('dense_wgrad writes row-major gw and a contiguous gb')
    lib = _lib.load()
    tw = tb = None
    for r in range(0, M, MAX_ROWS):
        m = min(MAX_ROWS, M - r)
        if r and tw is None:
            tw = torch.empty_like(gw)
            tb = None if gb is None else torch.empty_like(gb)
        ow, ob = (gw, gb) if r == 0 else (tw, tb)
        _lib.check(lib.scl_dense_wgrad(
            _lib.ptr(x[r:]), x.stride(0), _lib.ptr(gy[r:]), gy.stride(0),
            None if y is None else _lib.ptr(y[r:]), 0 if y is None else y.stride(0), m, K, N,
            _lib.ptr(ow), ow.stride(0), _lib.ptr(ob), _lib.stream_of(x)))
        if r:
            gw.add_(tw)
            if gb is not None:
                gb.add_(tb)


class _DenseFn(torch.autograd.Function):
    """One ``tf.layers.dense`` layer on the HIP kernels."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        y = dense_fwd(x, w, b, relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, w, b, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, b, y = ctx.saved_tensors
        gy = gy.contiguous()
        gx = dense_bwd_data(gy, y, w) if ctx.needs_input_grad[0] else None
        gw = gb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = nets._grad_out(w), nets._grad_out(b)
            dense_wgrad(x, gy, y, gw, gb)
            gw, gb = nets._grad_ret(gw, w), nets._grad_ret(gb, b)
        return gx, gw, gb, None


def dense(x, w, b, relu):
    """One layer: the HIP kernels on a device, plain torch float32 on the CPU."""
    if x.is_cuda:
        return _DenseFn.apply(x, w, b, relu)
    y = torch.addmm(b, x, w)
    return torch.relu(y) if relu else y


class DenseHead(torch.nn.Module):
    """The variables and the forward of one ``--reduction 1fc|2fc|3fc`` head."""

    def __init__(self, kind, in_dim, out_dim=512, seed=4321):
        super().__init__()
        self.kind, self.in_dim, self.out_dim = kind, int(in_dim), int(out_dim)
        if self.in_dim < 1 or self.out_dim < 1:
            raise ValueError('dense head needs in_dim, out_dim >= 1')
        self.specs = layer_specs(kind, self.in_dim, self.out_dim)
        g = torch.Generator().manual_seed(seed)
        for name, fin, units, _ in self.specs:
            limit = math.sqrt(6.0 / (fin + units))            # glorot_uniform_initializer
            k = torch.rand(fin, units, generator=g).mul_(2.0 * limit).sub_(limit)
            self.register_parameter(name + '_kernel', torch.nn.Parameter(k))
            self.register_parameter(name + '_bias', torch.nn.Parameter(torch.zeros(units)))

    def tf_variables(self):
        """[(TF variable name, parameter)] in creation order."""
        out = []
        for name, _, _, _ in self.specs:
            out.append((name + '/kernel', getattr(self, name + '_kernel')))
            out.append((name + '/bias', getattr(self, name + '_bias')))
        return out

    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.in_dim:
            raise ValueError('--reduction %s expects descriptors of width %d (fixed when the head '
                             'was built), got %s' % (self.kind, self.in_dim, tuple(x.shape)))
        x = x.float()
        for name, _, _, relu in self.specs:
            # (tf.layers.dropout after a ReLU layer: the identity, see the module docstring)
            x = dense(x, getattr(self, name + '_kernel'), getattr(self, name + '_bias'), relu)
        return x


def attach(model, kind, out_dim=512, in_dim=None, height=180, width=240, seed=4321):
    """Give ``model`` a dense head (``model.reduction_head``; on the model's device) and return it.
    ``in_dim`` defaults to the static width of the model's ``full_out`` at ``height`` x ``width``."""
    if in_dim is None:
        in_dim = head_in_dim(getattr(model, 'vlad_cores', 64), height, width)
    head = DenseHead(kind, in_dim, out_dim, seed=seed)
    model.reduction_head = head.to(next(model.parameters()).device)
    return model.reduction_head


def head_of(model):
    return getattr(model, 'reduction_head', None)

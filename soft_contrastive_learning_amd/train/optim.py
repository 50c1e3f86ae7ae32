"""The reference's optimisers (train/train.py:865-878) on torch's fused kernels.

`tf.train.AdamOptimizer(learning_rate)` (train/train.py:870; tensorflow==1.10.0, README.md:6 —
kernel ApplyAdam, non-Nesterov) updates

    lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    m   += (1 - beta1) * (g - m)
    v   += (1 - beta2) * (g * g - v)
    var -= lr_t * m / (sqrt(v) + epsilon)                   beta1 0.9, beta2 0.999, epsilon 1e-8

with epsilon OUTSIDE the bias correction ("epsilon hat" of the Adam paper, section 2).
`torch.optim.Adam` divides by sqrt(v / (1 - beta2^t)) + eps.  The two are the same formula with

    eps_torch(t) = epsilon / sqrt(1 - beta2^t)

— 31.6 x epsilon at the first step, 3.3 x after 100, 1.16 x after 1000.  At the reference's learning
rate (5e-6) and batch (25 images) most weights of the lower layers see gradients of 1e-8 … 1e-6:
there the denominators differ by that factor, i.e. a fixed-eps torch Adam takes steps up to
several times LARGER than the reference's during the first hundreds of steps.  `TFAdam` feeds
torch's fused kernel the step-dependent eps, which makes it `tf.train.AdamOptimizer` to rounding
(tests/test_optim.py against oracle/adam_np.py).

`tf.train.MomentumOptimizer(lr, 0.9)` (train/train.py:868): accum = 0.9 accum + g; var -= lr accum
is `torch.optim.SGD(momentum=0.9)` as it stands (dampening 0, no Nesterov).

`make_optimizer(..., impl='hip')` gives the same two updates as kernels of this package instead
(`HipAdam`, `HipMomentum`; csrc/optim.hip, scl_apply_adam / scl_apply_momentum): one launch over
all parameters, the float32 sequence of oracle/adam_np.py bit for bit — beta1_power / beta2_power
are float32 accumulators on the device, multiplied once per step as ApplyAdam's are, where
`TFAdam` carries `beta ** t` in double — and the same update under a captured graph, where
`TFAdam` falls back to torch's epsilon.  Float32 parameters on a HIP device only; the learning
rate and an optional skip word (`GradStats`: a non-finite gradient) are read on the device.
"""
import math

import numpy as np
import torch

from .. import _lib


class TFAdam(torch.optim.Adam):
    def __init__(self, params, lr, betas=(0.9, 0.999), epsilon=1e-8, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=epsilon, **kw)
        self.tf_epsilon = float(epsilon)
        self._t = None                    # steps taken; read from the state once (one device sync)

    def _steps_done(self):
        for g in self.param_groups:
            for p in g['params']:
                st = self.state.get(p)
                if st and 'step' in st:
                    return int(st['step'])
        return 0

    def eps_for_step(self, t, beta2):
        return self.tf_epsilon / math.sqrt(1.0 - beta2 ** t)

    @torch.no_grad()
    def step(self, closure=None):
        if self._t is None:
            self._t = self._steps_done()
        self._t += 1
        for g in self.param_groups:
            if g.get('capturable'):
                continue                  # a captured graph bakes eps in: plain torch Adam semantics
            g['eps'] = self.eps_for_step(self._t, g['betas'][1])
        return super().step(closure)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._t = None


def optim_chunks(n):
    """Workgroups that serve a segment of n elements (include/scl_hip.h, SclOptimSeg)."""
    return max(1, (n // 4 + _lib.OPTIM_CHUNK_GROUPS - 1) // _lib.OPTIM_CHUNK_GROUPS)


class _HipOptimizer(torch.optim.Optimizer):
    """What HipAdam and HipMomentum share: the device table of segments (csrc/optim.hip), the
    learning rate and the skip word on the device.

    ``lr_tensor``  device float32 [1]: what the kernel reads.  ``step()`` refreshes it when
                   ``param_groups[*]['lr']`` differs from the value last uploaded; between the
                   replays of a captured graph, fill it directly.
    ``skip_flag``  None, or a device word (int32 [1]): where it is non-zero, ``step()`` changes
                   nothing at all (``GradStats.flag`` is such a word).  Set it before capturing.

    The table is built on the first ``step()`` and again only when the addresses of a parameter,
    its gradient or a slot change, or a gradient appears or disappears (a parameter whose ``.grad``
    is None sits the step out, as in torch).  Apart from that a step allocates nothing and never
    waits for the device."""
    SLOTS = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        ps = [p for g in self.param_groups for p in g['params']]
        for p in ps:
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32
                    and p.is_contiguous() and p.device == ps[0].device):
                raise ValueError("impl='hip' updates contiguous float32 parameters on one HIP device; got %s on %s"
                                 % (getattr(p, 'dtype', type(p)), getattr(p, 'device', None)))
        self._dev = ps[0].device
        self._lr_uploaded = self._one_lr()
        self.lr_tensor = torch.full((1,), self._lr_uploaded, dtype=torch.float32, device=self._dev)
        self.skip_flag = None
        self._key = None
        self._table = None
        self._nseg = self._chunks = 0

    def _one_lr(self):
        lrs = {float(g['lr']) for g in self.param_groups}
        if len(lrs) != 1:
            raise ValueError('one learning rate for all parameter groups (one device scalar); got %s' % sorted(lrs))
        return lrs.pop()

    def _new_state(self, p, st):
        for name in self.SLOTS:
            st[name] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _build(self, rows, key):
        tab = np.zeros((len(rows), _lib.OPTIM_SEG_WORDS), dtype=np.int64)
        chunk = 0
        for r, (p, g, slots) in enumerate(rows):
            for t in (g,) + slots:
                if not (t.is_cuda and t.device == p.device and t.dtype == torch.float32
                        and t.is_contiguous() and t.numel() == p.numel()):
                    raise ValueError("impl='hip': gradients and slots are contiguous float32 tensors of the "
                                     "parameter's size on its device")
            tab[r, 0], tab[r, 1], tab[r, 2] = p.data_ptr(), g.data_ptr(), slots[0].data_ptr()
            tab[r, 3] = slots[1].data_ptr() if len(slots) > 1 else 0
            tab[r, 4], tab[r, 5] = p.numel(), chunk
            chunk += optim_chunks(p.numel())
        self._table = torch.from_numpy(tab).to(self._dev) if rows else None
        self._nseg, self._chunks, self._key = len(rows), chunk, key

    def _launch(self, lib, skip, stream):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lr = self._one_lr()
        if lr != self._lr_uploaded:
            self.lr_tensor.fill_(lr)
            self._lr_uploaded = lr
        rows, key = [], []
        for group in self.param_groups:
            for p in group['params']:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                st = self.state[p]
                if self.SLOTS[0] not in st:
                    self._new_state(p, st)
                slots = tuple(st[name] for name in self.SLOTS)
                rows.append((p, g, slots))
                key.append((p.data_ptr(), g.data_ptr(), p.numel()) + tuple(s.data_ptr() for s in slots))
        if key != self._key:
            self._build(rows, key)
        if not rows:
            return loss
        skip = self.skip_flag
        if skip is not None and not (skip.is_cuda and skip.device == self._dev and skip.numel() == 1
                                     and skip.element_size() == 4):
            raise ValueError('skip_flag is one 4-byte word on the device of the parameters')
        with torch.cuda.device(self._dev):
            _lib.check(self._launch(_lib.load(), _lib.ptr(skip), _lib.stream_of(self.lr_tensor)))
        # written behind autograd's back: say so, as an in-place torch op would
        torch._C._increment_version([p for p, _, _ in rows])
        return loss


class HipAdam(_HipOptimizer):
    """`tf.train.AdamOptimizer` as one HIP kernel over every parameter (scl_apply_adam): the update
    of oracle/adam_np.py bit for bit — float32 throughout, the two beta powers float32 accumulators
    that are multiplied once per step — under a captured graph as well as outside one.

    Slots under torch's names: ``state[p]['exp_avg']``, ``['exp_avg_sq']``; ``['step']`` is a view
    of the step word of the device state block (reading it waits for the device)."""
    SLOTS = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, lr, betas=(0.9, 0.999), epsilon=1e-8):
        super().__init__(params, dict(lr=lr, betas=tuple(betas), epsilon=epsilon))
        hyper = {(tuple(g['betas']), g['epsilon']) for g in self.param_groups}
        if len(hyper) != 1:
            raise ValueError('one (betas, epsilon) for all parameter groups')
        self.betas, self.epsilon = (float(betas[0]), float(betas[1])), float(epsilon)
        # SclOptimState: beta1_power, beta2_power (float32), step, ticket
        self._state = torch.zeros(4, dtype=torch.int32, device=self._dev)
        self.set_beta_powers(np.float32(self.betas[0]), np.float32(self.betas[1]), 0)

    def _new_state(self, p, st):
        super()._new_state(p, st)
        st['step'] = self._state[2]

    def beta_powers(self):
        """(beta1_power, beta2_power) as np.float32 — TensorFlow's accumulators, beta^(t+1) in
        float32 products after t steps — and t.  Waits for the device."""
        w = self._state.cpu().numpy()
        f = w.view(np.float32)
        return np.float32(f[0]), np.float32(f[1]), int(w[2])

    def set_beta_powers(self, b1p, b2p, steps):
        w = np.zeros(4, dtype=np.int32)
        w[:2] = np.array([b1p, b2p], dtype=np.float32).view(np.int32)
        w[2] = int(steps)
        self._state.copy_(torch.from_numpy(w))
        for st in self.state.values():
            if 'step' in st:
                st['step'] = self._state[2]

    def state_dict(self):
        sd = super().state_dict()
        b1p, b2p, steps = self.beta_powers()
        sd['beta_powers'] = (float(b1p), float(b2p), steps)
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if 'beta_powers' in state_dict:
            self.set_beta_powers(*state_dict['beta_powers'])

    def _launch(self, lib, skip, stream):
        return lib.scl_apply_adam(_lib.ptr(self._table), self._nseg, self._chunks, _lib.ptr(self._state),
                                  _lib.ptr(self.lr_tensor), self.betas[0], self.betas[1], self.epsilon,
                                  skip, stream)


class HipMomentum(_HipOptimizer):
    """`tf.train.MomentumOptimizer` (no Nesterov) as one HIP kernel (scl_apply_momentum):
    accum = accum * momentum + g; var -= lr * accum, each operation rounded on its own."""
    SLOTS = ('momentum_buffer',)

    def __init__(self, params, lr, momentum=0.9):
        super().__init__(params, dict(lr=lr, momentum=momentum))
        if len({float(g['momentum']) for g in self.param_groups}) != 1:
            raise ValueError('one momentum for all parameter groups')
        self.momentum = float(momentum)

    def _launch(self, lib, skip, stream):
        return lib.scl_apply_momentum(_lib.ptr(self._table), self._nseg, self._chunks,
                                      _lib.ptr(self.lr_tensor), self.momentum, skip, stream)


class GradStats:
    """scl_grad_stats over one flat float32 gradient buffer (parallel.GradBuckets.flat): ``run()``
    launches the pass on the current stream — ``flag`` is then 1 where the buffer holds a NaN or an
    infinity, the word an optimizer's ``skip_flag`` takes — and ``read()`` fetches
    (sum of squares of the finite entries, number of non-finite entries), which waits."""

    def __init__(self, flat):
        if not (flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() >= 1):
            raise ValueError('GradStats takes a contiguous float32 buffer on a HIP device')
        self.flat = flat
        self.out = torch.zeros(2, dtype=torch.float64, device=flat.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=flat.device)
        self._bytes = _lib.load().scl_grad_stats_workspace_bytes(flat.numel())
        self._work = _lib.workspace(self._bytes, flat.device)

    def run(self):
        with torch.cuda.device(self.flat.device):
            _lib.check(_lib.load().scl_grad_stats(
                _lib.ptr(self.flat), self.flat.numel(), _lib.ptr(self.out), _lib.ptr(self.flag),
                _lib.ptr(self._work), self._bytes, _lib.stream_of(self.flat)))

    def read(self):
        ss, bad = self.out.tolist()
        return ss, int(bad)


def make_optimizer(kind, params, lr, momentum=0.9, impl='torch'):
    """train/train.py:865-870: 'momentum' -> MomentumOptimizer, anything else -> AdamOptimizer.
    ``impl='hip'``: the same two updates as HIP kernels of this package (HipMomentum, HipAdam),
    for float32 parameters on a HIP device (ValueError otherwise)."""
    params = list(params)
    if impl == 'hip':
        if kind == 'momentum':
            return HipMomentum(params, lr=lr, momentum=momentum)
        return HipAdam(params, lr=lr)
    if impl != 'torch':
        raise ValueError("impl must be 'torch' or 'hip', got %r" % (impl,))
    if kind == 'momentum':
        return torch.optim.SGD(params, lr=lr, momentum=momentum)
    return TFAdam(params, lr=lr, fused=bool(params) and params[0].is_cuda)

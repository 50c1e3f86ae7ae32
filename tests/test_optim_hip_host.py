"""The HIP parameter update (csrc/optim.hip: scl_apply_adam, scl_apply_momentum, scl_grad_stats) as
far as a machine without a device can see it: the four symbols, the refusals that come back from the
host before any launch, and the opt-in switches above them (make_optimizer, the trainer's flags)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('scl_apply_adam', 'scl_apply_momentum', 'scl_grad_stats', 'scl_grad_stats_workspace_bytes')
NULL, SHAPE, WORKSPACE = -3, -1, -4


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_the_four_symbols_are_declared_exported_and_bound(lib):
    from soft_contrastive_learning_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'scl_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    diag = _lib.load(diag=True)
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(diag, name) is not None
    assert lib.scl_abi_version() == 12
    # the row and the state block as the header lays them out, and their Python mirrors
    assert 'SCL_OPTIM_CHUNK_GROUPS %d' % _lib.OPTIM_CHUNK_GROUPS in header
    row = re.search(r'typedef struct SclOptimSeg \{(.*?)\}', header, re.S).group(1)
    assert len([f for f in row.split(';') if f.strip()]) == _lib.OPTIM_SEG_WORDS


def test_the_update_is_refused_on_the_host(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    adam = lambda segs=p, nseg=1, total=1, state=p, lr=p: lib.scl_apply_adam(
        segs, nseg, total, state, lr, 0.9, 0.999, 1e-8, None, None)
    mom = lambda segs=p, nseg=1, total=1, lr=p: lib.scl_apply_momentum(segs, nseg, total, lr, 0.9, None, None)
    assert adam(segs=None) == NULL and adam(state=None) == NULL and adam(lr=None) == NULL
    assert mom(segs=None) == NULL and mom(lr=None) == NULL
    for f in (adam, mom):
        assert f(nseg=0) == SHAPE and f(nseg=-1) == SHAPE and f(nseg=(1 << 20) + 1, total=1 << 21) == SHAPE
        assert f(nseg=2, total=1) == SHAPE                   # fewer workgroups than rows
        assert f(total=(1 << 24) + 1) == SHAPE and f(total=0) == SHAPE
    # NULL comes before the shape, as in the other entry points
    assert adam(segs=None, nseg=0) == NULL and mom(lr=None, nseg=0) == NULL


def test_grad_stats_workspace_and_refusals(lib):
    ws = lib.scl_grad_stats_workspace_bytes
    assert ws(1) > 0 and ws(1 << 28) > 0 and ws(1) % 256 == 0 and ws(1 << 28) % 256 == 0
    assert ws(0) == 0 and ws(-5) == 0 and ws((1 << 40) + 1) == 0
    assert ws(1 << 28) >= ws(1) and ws(1 << 40) == ws(1 << 28)          # the partials are capped
    buf = ctypes.create_string_buffer(1 << 15)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd2, odd8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 8)
    stats = lambda g=p, n=1, out=p, flag=p, work=p, nbytes=ws(1): lib.scl_grad_stats(
        g, n, out, flag, work, nbytes, None)
    for kw in (dict(g=None), dict(out=None), dict(flag=None), dict(work=None)):
        assert stats(n=0, **kw) == NULL, kw
    assert stats(n=0) == SHAPE and stats(n=(1 << 40) + 1) == SHAPE and stats(g=odd2) == SHAPE
    assert stats(nbytes=ws(1) - 1) == WORKSPACE and stats(work=odd8) == WORKSPACE
    assert stats(n=1 << 28, nbytes=ws(1 << 28) - 1) == WORKSPACE


def test_make_optimizer_keeps_its_defaults_and_refuses_cpu_parameters_for_hip():
    from soft_contrastive_learning_amd.train import optim
    params = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))]
    adam = optim.make_optimizer('adam', params, 1e-3)
    assert type(adam) is optim.TFAdam and adam.defaults['fused'] is False
    assert type(optim.make_optimizer('momentum', params, 1e-2, 0.8)) is torch.optim.SGD
    assert type(optim.make_optimizer('adam', params, 1e-3, impl='torch')) is optim.TFAdam
    for kind in ('adam', 'momentum'):
        with pytest.raises(ValueError):
            optim.make_optimizer(kind, params, 1e-3, impl='hip')
    with pytest.raises(ValueError):
        optim.make_optimizer('adam', params, 1e-3, impl='triton')
    assert issubclass(optim.HipAdam, torch.optim.Optimizer) and issubclass(optim.HipMomentum, torch.optim.Optimizer)
    # a segment of n elements takes max(1, ceil(floor(n / 4) / 1024)) workgroups (include/scl_hip.h)
    assert [optim.optim_chunks(n) for n in (1, 3, 4, 4096, 4099, 4100, 1024 * 37 + 5)] == [1, 1, 1, 1, 1, 2, 10]


def test_skip_nonfinite_needs_the_hip_optimizer(monkeypatch):
    from soft_contrastive_learning_amd.train import train as T

    def no_device(*a, **k):
        raise AssertionError('the trainer touched the device before refusing')
    monkeypatch.setattr(torch.cuda, 'set_device', no_device)
    with pytest.raises(SystemExit) as e:
        T.main(['--skip_nonfinite', '1'])
    assert 'optimizer_impl' in str(e.value)
    with pytest.raises(SystemExit):
        T.main(['--skip_nonfinite', '1', '--optimizer_impl', 'torch'])
    flags = T.make_parser().parse_args([])
    assert flags.optimizer_impl == 'torch' and flags.skip_nonfinite == 0

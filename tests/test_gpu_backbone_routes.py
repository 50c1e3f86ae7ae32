"""Which kernel serves which convolution pass of the whole backbone, in launch order: the ordered
kernel names of one ``model.features`` forward and backward at the default switches equal the lists of
tests/golden/backbone_routes_v1.json, recorded by scripts/backbone_route_trace.py (``--golden``) BEFORE
the per-layer routing of model/nets.py was gathered into ``_fwd_route`` / ``_bwd_route`` — the
expectation comes from that earlier code, never from the code under test."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the switches a measurement may move (nets.autotune_side_wrw) at the values the lists were recorded with
DEFAULTS = {'USE_SIDE_WRW': True, 'USE_FUSED_FIRST_WRW': None, 'USE_SPLIT_FWD': None}


@pytest.fixture(scope='module')
def trace():
    spec = importlib.util.spec_from_file_location('backbone_route_trace',
                                                  os.path.join(ROOT, 'scripts', 'backbone_route_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'backbone_routes_v1.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('sink', [True, False], ids=['sink', 'autograd'])
@pytest.mark.parametrize('shape', [(2, 480, 640), (2, 180, 240), (3, 135, 241)], ids=lambda s: '%dx%dx%d' % s)
def test_launch_list_of_the_backbone(trace, golden, shape, sink, monkeypatch):
    from soft_contrastive_learning_amd.model import nets
    for k, v in DEFAULTS.items():
        monkeypatch.setattr(nets, k, v)
    launches, _, tensors = trace.run_case(nets, torch.device('cuda:0'), shape, sink=sink)
    assert launches == golden[trace.case_name(shape, sink)]
    assert all(bool(torch.isfinite(t).all()) for t in tensors.values())

"""The host side of the device resize: util/cv.py's plan (the tables csrc/frames.hip applies) against
the resampler it was cut out of, the launcher's refusals, and the callers' bookkeeping.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

from soft_contrastive_learning_amd.util import cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    """(sh, sw, kwargs of resize_linear): the named corners, then a seeded sweep."""
    cases = [
        (1, 1, dict(fx=1.0, fy=1.0)), (1, 1, dict(dsize=(3, 2))), (1, 1, dict(fx=4.0, fy=7.0)),
        (5, 1, dict(dsize=(1, 3))), (1, 5, dict(dsize=(3, 1))), (9, 13, dict(dsize=(1, 4))),   # dw = 1
        (7, 5, dict(fx=0.5, fy=0.5)), (8, 8, dict(fx=0.5, fy=0.5)), (4, 6, dict(fx=2.0, fy=2.0)),
        (33, 47, dict(dsize=(20, 9))), (33, 47, dict(dsize=(9, 20))), (12, 10, dict(fx=0.3, fy=1.7)),
        (960, 1280, dict(fx=240 / 1280.0, fy=240 / 1280.0)), (1280, 960, dict(fx=240 / 1280.0, fy=240 / 1280.0)),
    ]
    rng = np.random.default_rng(20240)
    for _ in range(40):
        sh, sw = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        if rng.random() < 0.5:
            fx, fy = float(rng.uniform(0.15, 3.0)), float(rng.uniform(0.15, 3.0))
            if int(np.rint(sw * fx)) < 1 or int(np.rint(sh * fy)) < 1:
                continue
            cases.append((sh, sw, dict(fx=fx, fy=fy)))
        else:
            cases.append((sh, sw, dict(dsize=(int(rng.integers(1, 90)), int(rng.integers(1, 90))))))
    return cases


CASES = _cases()


def _expected_axes(sh, sw, fx=None, fy=None, dsize=None):
    """resize_linear's own size rule and its two _axis calls."""
    if dsize is not None:
        dw, dh = int(dsize[0]), int(dsize[1])
        fx, fy = dw / float(sw), dh / float(sh)
    else:
        dw, dh = int(np.rint(sw * float(fx))), int(np.rint(sh * float(fy)))
    return dh, dw, cv._axis(dw, sw, float(fx), True), cv._axis(dh, sh, float(fy), False)


def test_plan_tables_are_the_axis_tables():
    for sh, sw, kw in CASES:
        plan = cv.resize_plan(sh, sw, **kw)
        dh, dw, xs, ys = _expected_axes(sh, sw, **kw)
        assert (plan.dh, plan.dw, plan.sh, plan.sw) == (dh, dw, sh, sw), (sh, sw, kw)
        for name, want in zip(('x0', 'x1', 'a0', 'a1', 'y0', 'y1', 'b0', 'b1'), tuple(xs) + tuple(ys)):
            got = getattr(plan, name)
            assert got.dtype == np.int32 and got.shape == (dw if name[0] in 'xa' else dh,), (name, sh, sw, kw)
            np.testing.assert_array_equal(got, want, err_msg='%s %s' % (name, (sh, sw, kw)))
        assert plan.xtab().shape == (4, dw) and plan.ytab().shape == (4, dh)
        assert plan.xtab().dtype == np.int32 and plan.xtab().flags.c_contiguous
        np.testing.assert_array_equal(plan.ytab()[3], ys[3])
    with pytest.raises(ValueError):
        cv.resize_plan(4, 4, 0.1, 0.1)                       # empty destination
    with pytest.raises(ValueError):
        cv.resize_plan(0, 4, 1.0, 1.0)


def _frozen_resize_linear(img, fx=None, fy=None, dsize=None):
    """resize_linear as it stood before the plan was cut out of it (kept here so that the test does
    not compare apply_plan with itself)."""
    flat = img.ndim == 2
    src = img[:, :, None] if flat else img
    dh, dw, (x0, x1, a0, a1), (y0, y1, b0, b1) = _expected_axes(src.shape[0], src.shape[1], fx, fy, dsize)

    def hpass(rows):
        return rows[:, x0].astype(np.int32) * a0[None, :, None] + rows[:, x1].astype(np.int32) * a1[None, :, None]
    s0, s1 = hpass(src[y0]), hpass(src[y1])
    out = (((b0[:, None, None] * (s0 >> 4)) >> 16) + ((b1[:, None, None] * (s1 >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[:, :, 0] if flat else out


def test_apply_plan_is_resize_linear():
    rng = np.random.default_rng(7)
    for sh, sw, kw in CASES:
        for shape in ((sh, sw), (sh, sw, 3)):
            img = rng.integers(0, 256, size=shape, dtype=np.uint8)
            got = cv.apply_plan(img, cv.resize_plan(sh, sw, **kw))
            assert got.dtype == np.uint8
            np.testing.assert_array_equal(got, cv.resize_linear(img, **kw), err_msg=str((shape, kw)))
            np.testing.assert_array_equal(got, _frozen_resize_linear(img, **kw), err_msg=str((shape, kw)))
    with pytest.raises(ValueError):
        cv.apply_plan(np.zeros((4, 5, 3), np.uint8), cv.resize_plan(5, 4, 1.0, 1.0))
    with pytest.raises(ValueError):
        cv.apply_plan(np.zeros((4, 5, 3), np.float32), cv.resize_plan(4, 5, 1.0, 1.0))


def _frozen_standard_size(img, h, w):
    import math
    scale = max(h / img.shape[0], w / img.shape[1])
    img = _frozen_resize_linear(img, scale, scale)
    top = math.floor((img.shape[0] - h) / 2.0)
    left = math.floor((img.shape[1] - w) / 2.0)
    return img[top:top + h, left:left + w, :]


@pytest.mark.parametrize('sh,sw', [(960, 1280), (1280, 960), (480, 640), (61, 83), (83, 61), (100, 100)])
def test_rule_plans_are_resize_img_and_standard_size(sh, sw):
    rng = np.random.default_rng(sh * 7 + sw)
    img = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    for max_size in (240, 80, 57):
        got = cv.apply_plan(img, cv.plan_resize_img(sh, sw, max_size))
        np.testing.assert_array_equal(got, cv.resize_img(img, max_size))
        scale = max_size / float(max(sh, sw))
        np.testing.assert_array_equal(got, _frozen_resize_linear(img, scale, scale))
        assert max(got.shape[:2]) == max_size
    # landscape target, portrait target (h=240, w=180 on 960 x 1280 is the 'achen' case), a square
    for h, w in ((180, 240), (240, 180), (45, 45), (30, 52)):
        plan = cv.plan_standard_size(sh, sw, h, w)
        assert (plan.dh, plan.dw) == (h, w)
        got = cv.apply_plan(img, plan)
        np.testing.assert_array_equal(got, cv.standard_size(img, h, w))
        np.testing.assert_array_equal(got, _frozen_standard_size(img, h, w))


def test_standard_size_plan_has_a_crop_origin():
    """480 x 640 -> cover 180 x 240 is exact (no crop); 960 x 1280 -> 240 x 180 cuts 70 columns a side."""
    full = cv.resize_plan(960, 1280, 0.25, 0.25)
    plan = cv.plan_standard_size(960, 1280, 240, 180)
    assert (full.dh, full.dw) == (240, 320)
    np.testing.assert_array_equal(plan.x0, full.x0[70:250])
    np.testing.assert_array_equal(plan.y0, full.y0)


def test_window_is_a_slice_of_the_result():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(33, 47, 3), dtype=np.uint8)
    plan = cv.resize_plan(33, 47, dsize=(20, 9))
    whole = cv.apply_plan(img, plan)
    for top, left, h, w in ((0, 0, 9, 20), (2, 3, 5, 11), (8, 19, 1, 1), (0, 7, 9, 1)):
        cut = plan.window(top, left, h, w)
        assert (cut.dh, cut.dw, cut.sh, cut.sw) == (h, w, 33, 47)
        np.testing.assert_array_equal(cv.apply_plan(img, cut), whole[top:top + h, left:left + w])
    for bad in ((-1, 0, 2, 2), (0, 0, 10, 20), (0, 15, 2, 6), (0, 0, 0, 3)):
        with pytest.raises(ValueError):
            plan.window(*bad)


# ---- the launcher -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_resize_launcher_refuses_on_the_host(lib):
    from soft_contrastive_learning_amd import _lib
    NULL, SHAPE = -3, -1
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 1)

    def call(src=p, n=2, sh=8, sw=8, c=3, xtab=p, ow=4, ytab=p, oh=4, kind=_lib.FRAMES_F32, out=p):
        return lib.scl_frames_resize(src, n, sh, sw, c, xtab, ow, ytab, oh, kind, out, None)

    # NULL operands — before the shape (n = 0 is refused as a shape)
    for kw in (dict(src=None), dict(xtab=None), dict(ytab=None), dict(out=None)):
        assert call(n=0, **kw) == NULL, kw
    assert call(c=2) == SHAPE and call(c=4) == SHAPE and call(c=0) == SHAPE
    assert call(n=0) == SHAPE and call(n=-1) == SHAPE and call(n=65536) == SHAPE
    assert call(sh=16385) == SHAPE and call(sw=16385) == SHAPE
    assert call(sh=0) == SHAPE and call(sw=0) == SHAPE and call(oh=0) == SHAPE and call(ow=-3) == SHAPE
    assert call(oh=16385) == SHAPE and call(ow=16385) == SHAPE
    assert call(kind=2) == SHAPE and call(kind=-1) == SHAPE
    assert call(out=odd) == SHAPE                                  # float32 at an odd address
    assert call(out=odd, kind=_lib.FRAMES_U8, n=0) == SHAPE        # (bytes may sit there: n decides)


def test_abi_stays_12(lib):
    from soft_contrastive_learning_amd import _lib
    assert lib.scl_abi_version() == 12 and _lib.ABI_VERSION == 12
    header = open(os.path.join(ROOT, 'include', 'scl_hip.h')).read()
    assert re.search(r'#define\s+SCL_ABI_VERSION\s+12\b', header)
    assert re.search(r'#define\s+SCL_FRAMES_U8\s+0\b', header) and _lib.FRAMES_U8 == 0
    assert re.search(r'#define\s+SCL_FRAMES_F32\s+1\b', header) and _lib.FRAMES_F32 == 1
    assert 'scl_frames_resize' in _lib.SIGNATURES


def test_a_cpu_device_is_refused():
    from soft_contrastive_learning_amd import _lib
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    with pytest.raises(_lib.SclError):
        DeviceResizer('cpu')


def test_batch_shapes_are_checked_on_the_host():
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    as_batch = DeviceResizer._as_batch
    u8 = lambda *s: np.zeros(s, np.uint8)
    assert as_batch(u8(5, 7)).shape == (1, 5, 7, 1)
    assert as_batch(u8(5, 7, 3)).shape == (1, 5, 7, 3)
    assert as_batch(u8(2, 5, 7, 1)).shape == (2, 5, 7, 1)
    assert as_batch([u8(5, 7, 3), u8(5, 7, 3)]).shape == (2, 5, 7, 3)
    assert as_batch([u8(5, 7)] * 3).shape == (3, 5, 7, 1)
    import torch
    assert tuple(as_batch(torch.zeros(5, 7, 3, dtype=torch.uint8)).shape) == (1, 5, 7, 3)
    for bad in (np.zeros((5, 7, 3), np.float32), u8(5, 7, 4), u8(5, 7, 2), u8(2, 5, 7, 4), u8(1, 2, 5, 7, 3),
                [u8(5, 7, 3), u8(7, 5, 3)], [], u8(0, 7, 3), torch.zeros(5, 7, 3), 'frame'):
        with pytest.raises(ValueError):
            as_batch(bad)


# ---- inference ----------------------------------------------------------------------------------
def test_inference_parser_knows_device_resize():
    from soft_contrastive_learning_amd.evaluation import inference
    parser = inference.build_parser()
    assert parser.parse_args([]).device_resize == 0
    assert parser.parse_args(['--device_resize', '1']).device_resize == 1


def _write_pngs(tmp_path, name, shapes):
    from PIL import Image

    from soft_contrastive_learning_amd.util import io
    rng = np.random.default_rng(11)
    frames, paths = [], []
    for k, (h, w) in enumerate(shapes):
        frames.append(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        paths.append('f%02d.png' % k)
        Image.fromarray(frames[-1]).save(str(tmp_path / paths[-1]))
    io.save_csv({'path': paths}, str(tmp_path / ('%s.csv' % name)))
    return frames


def test_csv_loader_returns_raw_frames_and_the_rule(tmp_path):
    from soft_contrastive_learning_amd.evaluation import inference
    shapes = [(24, 32), (32, 24)]
    want = {
        ('achen_q', 64, True): ('standard_size', dict(h=20, w=15)),
        ('achen_q', 0, True): ('standard_size', dict(h=20, w=15)),
        ('plain', 64, True): ('resize_img', dict(max_size=20)),
        ('plain', 64, False): ('none', {}),
        ('plain', 0, True): ('standard_size', dict(h=15, w=20)),
        ('plain', 0, False): ('standard_size', dict(h=15, w=20)),
    }
    raw = {name: _write_pngs(tmp_path, name, shapes) for name in ('achen_q', 'plain')}
    for (name, cores, rescale), (rule, kw) in want.items():
        args = (name, str(tmp_path), str(tmp_path), cores, rescale, 15, 20)
        dev_load, num = inference.csv_loader(*args, device_resize=True)
        host_load, num2 = inference.csv_loader(*args)
        assert num == num2 == 2
        for i in range(2):
            img, got_rule, got_kw = dev_load(i)
            assert img.dtype == np.uint8
            np.testing.assert_array_equal(img, raw[name][i])
            assert (got_rule, got_kw) == (rule, kw), (name, cores, rescale)
            # the rule, applied on the host, is what the loader returns without the flag
            np.testing.assert_array_equal(inference.size_on_host(img, got_rule, got_kw), host_load(i))

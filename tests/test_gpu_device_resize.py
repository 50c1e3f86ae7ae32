"""The device resize (csrc/frames.hip scl_frames_resize, util/device_cv.py) against util/cv.py, bit
for bit, and its callers: Localizer.prepare_raw / locate_raw and inference --device_resize."""
import pickle

import numpy as np
import pytest
import torch

from soft_contrastive_learning_amd.util import cv
from tests import util_data as U

pytestmark = pytest.mark.gpu

OUTS = [torch.uint8, torch.float32]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def resizer(dev):
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    return DeviceResizer(dev)


@pytest.fixture(scope="module")
def camera_frame():
    return np.random.default_rng(1280).integers(0, 256, size=(960, 1280, 3), dtype=np.uint8)


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _same(got, want_u8, out):
    """got: device [1 or n, oh, ow, c]; want_u8: util/cv's uint8 result(s) with the same layout."""
    assert got.dtype == out and got.is_cuda and tuple(got.shape) == want_u8.shape, (got.shape, want_u8.shape)
    want = torch.from_numpy(want_u8.astype(np.float32) if out == torch.float32 else want_u8)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('shape,kw', [
    ((7, 5, 3), dict(fx=0.5, fy=0.5)),            # dsize rounds 3.5 x 2.5 to even; last column clamped
    ((8, 8, 3), dict(fx=0.5, fy=0.5)),            # exact 2 x 2 means
    ((4, 6, 3), dict(fx=2.0, fy=2.0)),            # 1/4 : 3/4 mixes, edge weights zeroed
    ((1, 1, 3), dict(dsize=(3, 2))),
    ((5, 1, 1), dict(dsize=(3, 7))),              # a one-pixel axis: x1 clamped
    ((1, 5, 1), dict(dsize=(7, 3))),              # ... y1 clamped
    ((33, 47, 3), dict(dsize=(20, 9))),           # fx != fy, odd row bytes
    ((33, 47, 1), dict(dsize=(20, 9))),
])
def test_kernel_is_resize_linear(resizer, shape, kw, out):
    img = _rand(shape, sum(shape))
    got = resizer.resize_linear(img, out=out, **kw)
    _same(got, cv.resize_linear(img, **kw)[None], out)
    if shape[2] == 1:                             # the grey form [SH,SW] is the one-channel frame
        assert torch.equal(resizer.resize_linear(img[:, :, 0], out=out, **kw), got)


def test_half_size_of_even_frames_is_the_block_mean(resizer):
    img = _rand((8, 8, 3), 88)
    mean = (img.reshape(4, 2, 4, 2, 3).astype(np.int32).sum(axis=(1, 3)) + 2) >> 2
    _same(resizer.resize_linear(img, 0.5, 0.5), mean.astype(np.uint8)[None], torch.uint8)


@pytest.mark.parametrize('out', OUTS)
def test_camera_frame_through_the_loaders_rules(resizer, camera_frame, out):
    got = resizer.resize_img(camera_frame, 240, out=out)
    assert tuple(got.shape) == (1, 180, 240, 3)
    _same(got, cv.resize_img(camera_frame, 240)[None], out)
    portrait = np.ascontiguousarray(camera_frame.transpose(1, 0, 2))
    got = resizer.standard_size(portrait, h=240, w=180, out=out)
    assert tuple(got.shape) == (1, 240, 180, 3)
    _same(got, cv.standard_size(portrait, h=240, w=180)[None], out)


@pytest.mark.parametrize('out', OUTS)
def test_cover_and_crop_with_a_crop_origin(resizer, out):
    img = _rand((480, 640, 3), 480)
    _same(resizer.standard_size(img, 180, 240, out=out), cv.standard_size(img, 180, 240)[None], out)
    # 480 x 640 covers 180 x 240 exactly; these two cut rows, then columns, at a non-zero origin
    plan = cv.plan_standard_size(480, 640, 150, 240)
    assert plan.y0[0] > 0
    _same(resizer.standard_size(img, 150, 240, out=out), cv.standard_size(img, 150, 240)[None], out)
    plan = cv.plan_standard_size(480, 640, 180, 200)
    assert plan.x0[0] > 0
    _same(resizer.standard_size(img, 180, 200, out=out), cv.standard_size(img, 180, 200)[None], out)
    # a window of resize_linear is the slice
    got = resizer.resize_linear(img, dsize=(64, 48), window=(5, 9, 30, 41), out=out)
    _same(got, cv.resize_linear(img, dsize=(64, 48))[None, 5:35, 9:50], out)


@pytest.mark.parametrize('out', OUTS)
def test_a_batch_is_its_frames(resizer, dev, out):
    frames = _rand((3, 61, 83, 3), 61)
    want = np.stack([cv.resize_img(f, 40) for f in frames])
    got = resizer.resize_img(frames, 40, out=out)
    _same(got, want, out)
    for k in range(3):
        assert torch.equal(resizer.resize_img(frames[k], 40, out=out)[0], got[k])
    # the same frames as a list, as a host tensor, as a pinned host tensor, as a device tensor
    t = torch.from_numpy(frames)
    for form in (list(frames), t, t.pin_memory(), t.to(dev)):
        assert torch.equal(resizer.resize_img(form, 40, out=out), got)
    with pytest.raises(ValueError):
        resizer.resize_img([frames[0], frames[1][:, :-1]], 40)
    with pytest.raises(ValueError):
        resizer.resize_img(frames.astype(np.float32), 40)
    with pytest.raises(ValueError):
        resizer.resize_img(frames, 40, out=torch.float16)


def test_the_staging_buffer_is_reused_and_grows(dev):
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    r = DeviceResizer(dev)
    small, big = _rand((2, 20, 30, 3), 1), _rand((5, 20, 30, 3), 2)
    a = r.resize_img(small, 12, out=torch.uint8)
    first = r._staging.data_ptr()
    assert r._staging.is_pinned() and r._staging.numel() == small.size
    b = r.resize_img(small[::-1].copy(), 12, out=torch.uint8)
    assert r._staging.data_ptr() == first
    c = r.resize_img(big, 12, out=torch.uint8)
    assert r._staging.numel() == big.size
    d = r.resize_img(small, 12, out=torch.uint8)
    assert r._staging.numel() == big.size
    assert torch.equal(a, d) and torch.equal(a, b.flip(0))
    _same(c, np.stack([cv.resize_img(f, 12) for f in big]), torch.uint8)


def _tables(plan, dev):
    return (torch.from_numpy(plan.xtab()).to(dev), torch.from_numpy(plan.ytab()).to(dev))


def test_any_byte_alignment_of_source_and_output(dev):
    from soft_contrastive_learning_amd.util.device_cv import apply_tables
    frames = _rand((2, 33, 47, 3), 33)                    # 141-byte rows, 4653-byte frames
    plan = cv.resize_plan(33, 47, dsize=(20, 9))
    xtab, ytab = _tables(plan, dev)
    aligned = torch.from_numpy(frames).to(dev)
    want = apply_tables(aligned, xtab, ytab, torch.empty((2, 9, 20, 3), dtype=torch.uint8, device=dev))
    _same(want, np.stack([cv.apply_plan(f, plan) for f in frames]), torch.uint8)
    raw = torch.zeros(frames.size + 1, dtype=torch.uint8, device=dev)
    shifted = raw[1:].view(frames.shape)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 2 == 1 and shifted.is_contiguous()
    got = apply_tables(shifted, xtab, ytab, torch.empty((2, 9, 20, 3), dtype=torch.uint8, device=dev))
    assert torch.equal(got, want)
    room = torch.full((want.numel() + 2,), 7, dtype=torch.uint8, device=dev)
    out = room[1:-1].view(want.shape)
    assert out.data_ptr() % 2 == 1
    apply_tables(aligned, xtab, ytab, out)
    assert torch.equal(out, want)
    assert int(room[0]) == 7 and int(room[-1]) == 7       # nothing beside the output was written
    # float32 must be 4-byte aligned: the launcher refuses, nothing runs
    f32 = torch.zeros(want.numel() * 4 + 4, dtype=torch.uint8, device=dev)[1:]
    from soft_contrastive_learning_amd import _lib
    assert _lib.load().scl_frames_resize(
        _lib.ptr(aligned), 2, 33, 47, 3, _lib.ptr(xtab), 20, _lib.ptr(ytab), 9, _lib.FRAMES_F32,
        _lib.ptr(f32), None) == -1


def test_table_indices_are_clamped_to_the_frame(dev):
    """A wrong table gives the pixels of the clamped table — it never reads outside the frame."""
    from soft_contrastive_learning_amd.util.device_cv import apply_tables
    sh, sw = 33, 47
    frames = _rand((2, sh, sw, 3), 5)
    plan = cv.resize_plan(sh, sw, dsize=(20, 9))
    xs = [t.copy() for t in (plan.x0, plan.x1, plan.a0, plan.a1)]
    ys = [t.copy() for t in (plan.y0, plan.y1, plan.b0, plan.b1)]
    xs[0][0], xs[1][3], xs[0][-1], xs[1][-1] = -5, -5, sw + 7, sw + 7
    ys[0][0], ys[1][2], ys[0][-1], ys[1][-1] = -5, -5, sh + 7, sh + 7
    wrong = cv.ResizePlan(sh, sw, xs, ys)
    clamped = cv.ResizePlan(sh, sw, [np.clip(xs[0], 0, sw - 1), np.clip(xs[1], 0, sw - 1), xs[2], xs[3]],
                            [np.clip(ys[0], 0, sh - 1), np.clip(ys[1], 0, sh - 1), ys[2], ys[3]])
    xtab, ytab = _tables(wrong, dev)
    for out in OUTS:
        got = apply_tables(torch.from_numpy(frames).to(dev), xtab, ytab,
                           torch.empty((2, 9, 20, 3), dtype=out, device=dev))
        torch.cuda.synchronize()
        _same(got, np.stack([cv.apply_plan(f, clamped) for f in frames]), out)


def test_tables_are_uploaded_once_per_shape_and_rule(dev):
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    r = DeviceResizer(dev)
    a, b = _rand((61, 83, 3), 1), _rand((61, 83, 3), 2)
    first = r.resize_img(a, 40)
    assert r.table_uploads == 1
    again = r.resize_img(a, 40)
    r.resize_img(b, 40, out=torch.uint8)
    r.resize_img(np.stack([a, b]), 40)
    assert r.table_uploads == 1 and torch.equal(first, again)
    r.resize_img(a, 41)
    r.standard_size(a, 30, 40)
    r.resize_img(_rand((83, 61, 3), 3), 40)
    assert r.table_uploads == 4
    r.standard_size(b, 30, 40)
    assert r.table_uploads == 4


def test_two_resizers_on_two_streams(dev):
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    frames = _rand((3, 61, 83, 3), 9)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    resizers = [DeviceResizer(dev), DeviceResizer(dev)]
    got = []
    for _ in range(2):
        for s, r in zip(streams, resizers):
            with torch.cuda.stream(s):
                got.append(r.resize_img(frames, 40))
    torch.cuda.synchronize()
    want = np.stack([cv.resize_img(f, 40) for f in frames])
    for g in got:
        _same(g, want, torch.float32)


def test_work_is_accounted(resizer):
    from soft_contrastive_learning_amd.model import nets
    from soft_contrastive_learning_amd.util.device_cv import kernel_bytes
    old, nets.WORK_LOG = nets.WORK_LOG, {}
    try:
        resizer.resize_img(_rand((2, 61, 83, 3), 4), 40)
        log = nets.WORK_LOG
    finally:
        nets.WORK_LOG = old
    oh, ow = cv.resize_img(np.zeros((61, 83, 3), np.uint8), 40).shape[:2]
    assert log['frames_resize_kernel'] == [1, 0.0, kernel_bytes(2, oh, ow, 3, 4)]


# ---- Localizer ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def located(dev):
    """The tiny model and track of test_gpu_retrieval_index.py::test_locate_images; ``raw`` are camera
    frames of 128 x 160 (the 64 x 80 test images up-sized on the host), the references are embedded
    from the HOST-resized frames."""
    from soft_contrastive_learning_amd.evaluation import localize
    from soft_contrastive_learning_amd.evaluation.inference import extract_features
    from soft_contrastive_learning_amd.model import nets
    model = nets.VGG16NetVLAD().to(dev).eval()
    small = np.clip(np.rint(U.pose_images(50, 64, 80)), 0, 255).astype(np.uint8)
    raw = np.stack([cv.resize_linear(f, 2.0, 2.0) for f in small])
    assert raw.shape == (50, 128, 160, 3) and raw.dtype == np.uint8
    host = np.stack([cv.resize_img(f, 80) for f in raw]).astype(np.float32)
    feats = extract_features(model, lambda i: host[i], 50, images_per_pass=10, device=dev, loader_threads=1)
    ref_xy = np.stack([0.5 * np.arange(50), 0.1 * np.random.default_rng(5).standard_normal(50)], 1)
    loc = localize.Localizer(np.stack(feats), ref_xy, model=model, n=3, device=dev)
    return loc, raw, host, ref_xy


def test_prepare_raw_is_the_host_resized_batch(located):
    loc, raw, host, _ = located
    got = loc.prepare_raw(raw, max_size=80)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (50, 64, 80, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(host))
    one = loc.prepare_raw(raw[7], max_size=80)
    assert torch.equal(one.cpu()[0], torch.from_numpy(host[7]))
    cover = loc.prepare_raw(raw[:2], rule='standard_size', h=40, w=64)
    want = np.stack([cv.standard_size(f, 40, 64) for f in raw[:2]]).astype(np.float32)
    assert torch.equal(cover.cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError):
        loc.prepare_raw(raw[:2], rule='bicubic')
    with pytest.raises(ValueError):
        loc.prepare_raw(raw[:2], rule='none', max_size=80)


def test_prepare_raw_default_is_240(located):
    loc, raw, _, _ = located
    want = np.stack([cv.resize_img(f, 240) for f in raw[:2]]).astype(np.float32)
    assert want.shape == (2, 192, 240, 3)
    assert torch.equal(loc.prepare_raw(raw[:2]).cpu(), torch.from_numpy(want))


def test_locate_raw_names_its_frames(located):
    loc, raw, host, ref_xy = located
    idx, fd, xy = loc.locate_raw(raw[:4], max_size=80)
    assert idx.shape == (4, 3) and xy.shape == (4, 3, 2)
    assert list(idx[:, 0]) == [0, 1, 2, 3]
    np.testing.assert_array_equal(xy[:, 0], ref_xy[:4])
    # the input tensor is equal (test_prepare_raw_is_the_host_resized_batch), so the distances get
    # no tolerance of their own: the host-resized frames name the same references
    idx2, _, _ = loc.locate(host[:4])
    np.testing.assert_array_equal(idx, idx2)
    assert float(fd[:, 0].max()) < 1e-3, fd[:, 0]


def test_rule_none_only_widens(located):
    loc, raw, _, _ = located
    small = np.ascontiguousarray(raw[:3, ::2, ::2])                 # 64 x 80 uint8, used as they are
    wide = torch.from_numpy(small.astype(np.float32))
    assert torch.equal(loc.prepare_raw(small, rule='none').cpu(), wide)
    (idx, _, xy), (idx2, _, xy2) = loc.locate_raw(small, rule='none'), loc.locate(wide)
    np.testing.assert_array_equal(idx, idx2)
    np.testing.assert_array_equal(xy, xy2)


# ---- inference ----------------------------------------------------------------------------------
def _write_set(root, name, shapes):
    from soft_contrastive_learning_amd.util import io
    rng = np.random.default_rng(96)
    paths = []
    for k, (h, w) in enumerate(shapes):
        paths.append('%s_%02d.png' % (name, k))
        io.save_img(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), root / paths[-1])
    io.save_csv({'path': paths}, str(root / ('%s.csv' % name)))


def _run_inference(root, name, out_name, device_resize, monkeypatch):
    """-> (the pickle's list, the float32 batches handed to the network, in order)."""
    from soft_contrastive_learning_amd.evaluation import inference
    from soft_contrastive_learning_amd.model import nets
    batches, real = [], nets.output

    def recording(batch, model=None):
        assert batch.is_cuda and batch.dtype == torch.float32
        batches.append(batch.cpu())
        return real(batch, model=model)
    monkeypatch.setattr(nets, 'output', recording)
    inference.main(['--set', name, '--csv_root', str(root), '--img_root', str(root), '--out_root', str(root / 'out'),
                    '--out_name', out_name, '--images_per_pass', '4', '--large_side', '64', '--small_side', '48',
                    '--device_resize', str(device_resize)])
    monkeypatch.setattr(nets, 'output', real)
    return pickle.load(open(str(root / 'out' / ('%s_%s.pickle' % (name, out_name))), 'rb')), batches


def _assert_same_product(host, device):
    """Two runs with --device_resize 0 already differ in the last bits of the descriptors on the GPU
    (the library convolutions at these tiny tile counts do not repeat: measured, 5e-9 absolute on
    unit-norm descriptors), so the pickles are compared through what decides them: the float32
    batches handed to the network are EQUAL, batch by batch.  The descriptors get the tolerance the
    suite uses for one frame in two passes (test_gpu_callers.py)."""
    (host_feats, host_batches), (dev_feats, dev_batches) = host, device
    assert len(host_batches) == len(dev_batches) == 4
    for a, b in zip(host_batches, dev_batches):
        assert a.shape == b.shape == (4, 48, 64, 3)
        assert torch.equal(a, b)
    assert len(host_feats) == len(dev_feats) == 12
    for a, b in zip(host_feats, dev_feats):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (32768,)
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)


def test_inference_writes_the_same_pickle(dev, tmp_path, capsys, monkeypatch):
    _write_set(tmp_path, 'even', [(96, 128)] * 12)
    host = _run_inference(tmp_path, 'even', 'host', 0, monkeypatch)
    assert 'device_resize' not in capsys.readouterr().out
    device = _run_inference(tmp_path, 'even', 'device', 1, monkeypatch)
    assert 'device_resize: 0 of 4 batches sized on the host' in capsys.readouterr().out
    _assert_same_product(host, device)


def test_inference_sizes_a_mixed_batch_on_the_host(dev, tmp_path, capsys, monkeypatch):
    # frame 5 has another size (and the same 48 x 64 result): its batch of four goes the host's way
    _write_set(tmp_path, 'mixed', [(96, 128)] * 5 + [(192, 256)] + [(96, 128)] * 6)
    host = _run_inference(tmp_path, 'mixed', 'host', 0, monkeypatch)
    capsys.readouterr()
    device = _run_inference(tmp_path, 'mixed', 'device', 1, monkeypatch)
    assert 'device_resize: 1 of 4 batches sized on the host' in capsys.readouterr().out
    _assert_same_product(host, device)

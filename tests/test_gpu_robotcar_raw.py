"""Raw Bayer frames on the device (csrc/frames.hip scl_frames_debayer, DeviceResizer.debayer) against
the definition of util/robotcar.py — byte for byte, no tolerance — alone and fused with the loaders'
resize, and its callers: Localizer.prepare_raw(bayer=...), inference --bayer, the robotcar command."""
import pickle

import numpy as np
import pytest
import torch

from soft_contrastive_learning_amd.util import cv, robotcar
from tests import robotcar_data as D

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


def _same(got, want_u8, out=torch.uint8):
    assert got.dtype == out and got.is_cuda and tuple(got.shape) == want_u8.shape, (got.shape, want_u8.shape)
    want = torch.from_numpy(want_u8.astype(np.float32) if out == torch.float32 else want_u8)
    assert torch.equal(got.cpu(), want)


def _host(raw, pattern, lut, border):
    return np.stack([robotcar.load_image_np(f, pattern, lut, border) for f in raw])


@pytest.mark.parametrize('sh,sw', D.SHAPES)
def test_bytes_are_load_image_np(resizer, sh, sw):
    raw = D.raw_frames(3, sh, sw)
    assert not np.array_equal(raw[0], raw[1]) and not np.array_equal(raw[1], raw[2])
    luts = [None] + [D.mixed_lut(sh, sw, seed) for seed in range(5 if sh * sw <= 12 else 1)]
    for pattern in robotcar.PATTERNS:
        for border in robotcar.BORDERS:
            for lut in luts:
                want = _host(raw, pattern, lut, border)
                _same(resizer.debayer(raw, pattern, lut, border), want)
                _same(resizer.debayer(raw[1], pattern, lut, border), want[1:2])
    # the same frames as a list and as a device tensor; the float32 output is the byte widened
    got = resizer.debayer(raw, 'gbrg', luts[1])
    assert torch.equal(resizer.debayer(list(raw), 'gbrg', luts[1]), got)
    assert torch.equal(resizer.debayer(torch.from_numpy(raw).to(got.device), 'gbrg', luts[1]), got)
    wide = resizer.debayer(raw, 'gbrg', luts[1], out=torch.float32)
    assert wide.dtype == torch.float32 and torch.equal(wide, got.float())


def test_the_all_255_frame_wraps_under_reflect(resizer):
    raw = D.raw_frames(1, 6, 8)
    got = resizer.debayer(raw, 'gbrg', None, 'reflect').cpu().numpy()
    assert got.min() == 573 - 512 and got[0, 1:-1, 1:-1].min() == 255
    assert resizer.debayer(raw, 'gbrg', None, 'mirror').cpu().numpy().min() == 255


def test_any_byte_address_of_the_raw_frames(dev):
    from soft_contrastive_learning_amd.util.device_cv import debayer_tables
    sh, sw = 7, 9                                              # 63-byte frames
    raw = D.raw_frames(3, sh, sw, seed=4)
    lut = torch.from_numpy(D.mixed_lut(sh, sw)).to(dev)
    want = _host(raw, 'grbg', lut.cpu().numpy(), 'reflect')
    room = torch.zeros(raw.size + 1, dtype=torch.uint8, device=dev)
    shifted = room[1:].view(raw.shape)
    shifted.copy_(torch.from_numpy(raw))
    assert shifted.data_ptr() % 2 == 1 and shifted.is_contiguous()
    for out in OUTS:
        got = debayer_tables(shifted, 'grbg', 'reflect', lut, None, None,
                             torch.empty((3, sh, sw, 3), dtype=out, device=dev))
        _same(got, want, out)
    # a uint8 output at an odd address, with nothing written beside it
    guard = torch.full((want.size + 2,), 7, dtype=torch.uint8, device=dev)
    out = guard[1:-1].view(want.shape)
    debayer_tables(shifted, 'grbg', 'reflect', lut, None, None, out)
    _same(out, want)
    assert int(guard[0]) == 7 and int(guard[-1]) == 7


def test_a_wrong_table_gives_pixels_not_reads_outside_the_frame(resizer, dev):
    """Coordinates far outside, infinite or NaN are outside the frame: zeros, as on the host.  Resize
    tables with indices outside the frame give the pixels of the clamped tables."""
    from soft_contrastive_learning_amd.util.device_cv import debayer_tables
    sh, sw = 33, 47
    raw = D.raw_frames(2, sh, sw)
    lut = D.mixed_lut(sh, sw)
    lut[:, 5:12] = [[1e300, -1e300, np.inf, -np.inf, 2.0 ** 40, -2.0 ** 40, np.nan], [3.0] * 7]
    lut[1, 20:24] = [np.inf, -2.0 ** 31, 2.0 ** 31, 1e18]
    full = _host(raw, 'gbrg', lut, 'mirror')
    assert (full.reshape(2, -1, 3)[:, 5:12] == 0).all()
    _same(resizer.debayer(raw, 'gbrg', lut, 'mirror'), full)
    plan = cv.resize_plan(sh, sw, dsize=(20, 9))
    xs = [t.copy() for t in (plan.x0, plan.x1, plan.a0, plan.a1)]
    ys = [t.copy() for t in (plan.y0, plan.y1, plan.b0, plan.b1)]
    xs[0][0], xs[1][3], xs[0][-1], xs[1][-1] = -5, -5, sw + 7, sw + 7
    ys[0][0], ys[1][2], ys[0][-1], ys[1][-1] = -5, -5, sh + 7, sh + 7
    wrong = cv.ResizePlan(sh, sw, xs, ys)
    clamped = cv.ResizePlan(sh, sw, [np.clip(xs[0], 0, sw - 1), np.clip(xs[1], 0, sw - 1), xs[2], xs[3]],
                            [np.clip(ys[0], 0, sh - 1), np.clip(ys[1], 0, sh - 1), ys[2], ys[3]])
    got = debayer_tables(torch.from_numpy(raw).to(dev), 'gbrg', 'mirror', torch.from_numpy(lut).to(dev),
                         torch.from_numpy(wrong.xtab()).to(dev), torch.from_numpy(wrong.ytab()).to(dev),
                         torch.empty((2, 9, 20, 3), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    _same(got, np.stack([cv.apply_plan(f, clamped) for f in full]))


# ---- fused with the resize -------------------------------------------------------------------------
def _fused_case(resizer, raw, pattern, lut, border, rule, kw, plan):
    """The fused launch == scl_frames_resize on the device's full-size bytes == the host chain."""
    from soft_contrastive_learning_amd.util.device_cv import apply_tables
    full = resizer.debayer(raw, pattern, lut, border)
    host_full = _host(raw, pattern, lut, border)
    _same(full, host_full)
    want = np.stack([cv.apply_plan(f, plan) for f in host_full])
    xtab, ytab = (torch.from_numpy(t).to(full.device) for t in (plan.xtab(), plan.ytab()))
    for out in OUTS:
        got = resizer.debayer(raw, pattern, lut, border, rule, out, **kw)
        two = apply_tables(full, xtab, ytab, torch.empty(got.shape, dtype=out, device=full.device))
        assert torch.equal(got, two)
        _same(got, want, out)
    return want


@pytest.mark.parametrize('border', robotcar.BORDERS)
@pytest.mark.parametrize('pattern', robotcar.PATTERNS)
def test_fused_route_is_the_resize_of_the_bytes(resizer, pattern, border):
    sh, sw = 96, 128
    raw = D.raw_frames(3, sh, sw, seed=9)
    for lut in (D.mixed_lut(sh, sw), D.smooth_lut(sh, sw), None):
        want = _fused_case(resizer, raw, pattern, lut, border, 'resize_img', dict(max_size=24),
                           cv.plan_resize_img(sh, sw, 24))
        assert want.shape == (3, 18, 24, 3)
        _fused_case(resizer, raw, pattern, lut, border, 'standard_size', dict(h=18, w=24),
                    cv.plan_standard_size(sh, sw, 18, 24))
    _fused_case(resizer, raw[:1], pattern, None, border, 'standard_size', dict(h=20, w=16),
                cv.plan_standard_size(sh, sw, 20, 16))            # a crop origin in x


def test_camera_frame_with_a_lens_like_table(resizer):
    raw = np.random.default_rng(1280).integers(0, 256, size=(1, 960, 1280), dtype=np.uint8)
    lut = D.smooth_lut(960, 1280, seed=1)
    want = _fused_case(resizer, raw, 'gbrg', lut, 'reflect', 'resize_img', dict(max_size=240),
                       cv.plan_resize_img(960, 1280, 240))
    assert want.shape == (1, 180, 240, 3)
    with pytest.raises(ValueError):
        resizer.debayer(raw, 'gbrg', lut, rule='bicubic')
    with pytest.raises(ValueError):
        resizer.debayer(raw, 'gbrg', lut, rule='none', max_size=240)
    with pytest.raises(ValueError):
        resizer.debayer(raw, 'rgbg', lut)
    with pytest.raises(ValueError):
        resizer.debayer(raw, 'gbrg', lut, border='wrap')
    with pytest.raises(ValueError, match='Incorrect image size for camera model'):
        resizer.debayer(raw[:, :-2], 'gbrg', lut)
    with pytest.raises(ValueError):
        resizer.debayer(np.repeat(raw[..., None], 3, axis=3), 'gbrg', lut)      # demosaiced already
    with pytest.raises(ValueError):
        resizer.debayer(raw, 'gbrg', lut.astype(np.float32))


def test_tables_are_uploaded_once(dev):
    from soft_contrastive_learning_amd.util.device_cv import DeviceResizer
    r = DeviceResizer(dev)
    raw = D.raw_frames(2, 96, 128)
    lut, other = D.mixed_lut(96, 128), D.smooth_lut(96, 128)
    a = r.debayer(raw, 'gbrg', lut, rule='resize_img', max_size=24)
    b = r.debayer(raw[:1], 'gbrg', lut, rule='resize_img', max_size=24)
    assert r.lut_uploads == 1 and r.table_uploads == 1 and torch.equal(a[:1], b)
    r.debayer(raw, 'rggb', lut)                                   # full size: the same table, no plan
    r.resize_img(np.zeros((96, 128, 3), np.uint8), 24)            # the plan debayer uploaded serves resize_img
    assert r.lut_uploads == 1 and r.table_uploads == 1
    r.debayer(raw, 'gbrg', other)
    r.debayer(raw, 'gbrg', None)
    assert r.lut_uploads == 2
    r.debayer(raw, 'gbrg', lut)
    assert r.lut_uploads == 2


def test_work_is_accounted(resizer):
    from soft_contrastive_learning_amd.model import nets
    from soft_contrastive_learning_amd.util.device_cv import debayer_bytes
    raw, lut = D.raw_frames(2, 96, 128), D.mixed_lut(96, 128)
    old, nets.WORK_LOG = nets.WORK_LOG, {}
    try:
        resizer.debayer(raw, 'gbrg', lut, rule='resize_img', out=torch.float32, max_size=24)
        resizer.debayer(raw, 'gbrg', None)
        log = nets.WORK_LOG
    finally:
        nets.WORK_LOG = old
    fused = 4 * 18 * 24 * (16 + 2 * 16) + 3 * 2 * 18 * 24 * 4 + 16 * (18 + 24)
    full = 96 * 128 * (2 * 16) + 3 * 2 * 96 * 128
    assert debayer_bytes(2, 96, 128, 18, 24, 4, True, True) == fused
    assert debayer_bytes(2, 96, 128, 96, 128, 1, False, False) == full
    assert log['frames_debayer_kernel'] == [2, 0.0, float(fused + full)]


# ---- Localizer -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def localizer(dev):
    from soft_contrastive_learning_amd.evaluation import localize
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((64, 256), dtype=np.float32)
    return localize.Localizer(ref, np.stack([np.arange(64.0), np.zeros(64)], 1), n=3, device=dev)


def test_prepare_raw_without_bayer_is_unchanged(localizer):
    frames = np.random.default_rng(8).integers(0, 256, size=(2, 96, 128, 3), dtype=np.uint8)
    want = np.stack([cv.resize_img(f, 240) for f in frames]).astype(np.float32)
    got = localizer.prepare_raw(frames)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), torch.from_numpy(want))
    want = np.stack([cv.standard_size(f, 18, 24) for f in frames]).astype(np.float32)
    assert torch.equal(localizer.prepare_raw(frames, 'standard_size', h=18, w=24).cpu(), torch.from_numpy(want))
    assert torch.equal(localizer.prepare_raw(frames, rule='none').cpu(), torch.from_numpy(frames.astype(np.float32)))


def test_prepare_raw_with_bayer_is_the_fused_route(localizer, resizer):
    raw, lut = D.raw_frames(3, 96, 128, seed=2), D.smooth_lut(96, 128)
    got = localizer.prepare_raw(raw, max_size=24, bayer='gbrg', lut=lut)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 18, 24, 3)
    assert torch.equal(got, resizer.debayer(raw, 'gbrg', lut, 'reflect', 'resize_img', torch.float32, max_size=24))
    host = np.stack([cv.resize_img(f, 24) for f in _host(raw, 'gbrg', lut, 'reflect')])
    _same(got, host, torch.float32)
    mirror = localizer.prepare_raw(raw, 'standard_size', bayer='rggb', lut=None, border='mirror', h=18, w=24)
    host = np.stack([cv.standard_size(f, 18, 24) for f in _host(raw, 'rggb', None, 'mirror')])
    _same(mirror, host, torch.float32)
    before = localizer._resizer.lut_uploads
    localizer.prepare_raw(raw[:1], max_size=24, bayer='gbrg', lut=lut)
    assert localizer._resizer.lut_uploads == before >= 1


# ---- the command lines -----------------------------------------------------------------------------
def _write_raw_set(root, name, count, sh=96, sw=128):
    from PIL import Image

    from soft_contrastive_learning_amd.util import io
    raw = D.raw_frames(count, sh, sw, seed=6)
    paths = []
    for k, f in enumerate(raw):
        paths.append('cam/%s_%02d.png' % (name, k))
        (root / 'cam').mkdir(exist_ok=True)
        Image.fromarray(f).save(str(root / paths[-1]))
    io.save_csv({'path': paths}, str(root / ('%s.csv' % name)))
    return raw, paths


def test_inference_takes_raw_frames(dev, tmp_path, monkeypatch):
    from soft_contrastive_learning_amd.evaluation import inference
    from soft_contrastive_learning_amd.model import nets
    raw, _ = _write_raw_set(tmp_path, 'rawset', 4)
    lut = D.smooth_lut(96, 128)
    robotcar.save_distortion_lut(lut, tmp_path / 'lut.bin')
    batches, real = [], nets.output

    def recording(batch, model=None):
        batches.append(batch.cpu())
        return real(batch, model=model)
    monkeypatch.setattr(nets, 'output', recording)
    inference.main(['--set', 'rawset', '--csv_root', str(tmp_path), '--img_root', str(tmp_path),
                    '--out_root', str(tmp_path / 'out'), '--images_per_pass', '4', '--large_side', '64',
                    '--device_resize', '1', '--bayer', 'gbrg', '--distortion_lut', str(tmp_path / 'lut.bin'),
                    '--bayer_border', 'mirror'])
    monkeypatch.setattr(nets, 'output', real)
    feats = pickle.load(open(str(tmp_path / 'out' / 'rawset_scl_amd.pickle'), 'rb'))
    assert len(feats) == 4 and feats[0].shape == (32768,) and feats[0].dtype == np.float32
    want = np.stack([cv.resize_img(f, 64) for f in _host(raw, 'gbrg', lut, 'mirror')]).astype(np.float32)
    assert len(batches) == 2 and torch.equal(batches[0], torch.from_numpy(want))


def test_robotcar_command_writes_the_sized_frames_and_exposures(dev, tmp_path, capsys):
    from soft_contrastive_learning_amd.util import io
    src = tmp_path / 'in'
    src.mkdir()
    raw, paths = _write_raw_set(src, 'f', 5)
    (src / 'cam' / 'broken.png').write_bytes(b'not a png')
    lut = D.smooth_lut(96, 128)
    robotcar.save_distortion_lut(lut, tmp_path / 'lut.bin')
    rows, skipped = robotcar.main(['--in_dir', str(src), '--out_dir', str(tmp_path / 'out'), '--distortion_lut',
                                   str(tmp_path / 'lut.bin'), '--max_side', '24', '--batch', '2'])
    assert skipped == ['cam/broken.png'] and 'skipped cam/broken.png' in capsys.readouterr().out
    want = [cv.resize_img(f, 24) for f in _host(raw, 'gbrg', lut, 'reflect')]
    assert [r for r, _ in rows] == paths
    table = io.load_csv(str(tmp_path / 'out' / 'exposure.csv'))
    assert table['path'] == paths
    for rel, w, (_, e), text in zip(paths, want, rows, table['exposure']):
        np.testing.assert_array_equal(io.load_img(str(tmp_path / 'out' / rel)), w)
        assert e == int(w.sum(dtype=np.int64)) == int(text)

"""The host side of the raw-frame route (util/robotcar.py): the definition against the scipy functions the
RobotCar SDK calls — equal bit for bit, no tolerance —, the table file, the launcher's refusals and the
refusals of the command lines.  No device."""
import ctypes

import numpy as np
import pytest

from soft_contrastive_learning_amd.util import robotcar
from tests import robotcar_data as D


# ---- the definition against scipy ------------------------------------------------------------------
def _sdk_demosaic(raw, pattern, border):
    """demosaicing_CFA_Bayer_bilinear as the SDK's dependency writes it, on scipy.ndimage.convolve."""
    from scipy.ndimage import convolve
    cfa = raw.astype(np.float64)
    r_m, g_m, b_m = (m.astype(np.float64) for m in robotcar.masks(raw.shape[0], raw.shape[1], pattern))
    h_g = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=np.float64) / 4
    h_rb = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.float64) / 4
    return np.stack([convolve(cfa * r_m, h_rb, mode=border), convolve(cfa * g_m, h_g, mode=border),
                     convolve(cfa * b_m, h_rb, mode=border)], axis=2)


def _sdk_undistort(img, lut):
    """CameraModel.undistort: map_coordinates(order=1) per channel, the table as the file has it."""
    from scipy.ndimage import map_coordinates
    sh, sw = img.shape[:2]
    cols, rows = lut[0].reshape(sh, sw), lut[1].reshape(sh, sw)
    return np.stack([map_coordinates(img[:, :, c], [rows, cols], order=1) for c in range(3)], axis=2)


def test_masks_follow_the_pattern_string():
    m = robotcar.masks(4, 6, 'gbrg')
    assert m.sum(axis=0).min() == 1 == m.sum(axis=0).max()
    assert m[1, 0, 0] and m[2, 0, 1] and m[0, 1, 0] and m[1, 1, 1]          # g b / r g
    m = robotcar.masks(3, 3, 'rggb')
    assert m[0, 0, 0] and m[1, 0, 1] and m[1, 1, 0] and m[2, 1, 1] and m[0, 2, 2]
    assert robotcar.STEREO_PATTERN == 'gbrg' and robotcar.MONO_PATTERN == 'rggb'
    assert sorted(robotcar.PATTERNS) == ['bggr', 'gbrg', 'grbg', 'rggb']
    with pytest.raises(ValueError):
        robotcar.masks(4, 4, 'rgbg')
    with pytest.raises(ValueError):
        robotcar.demosaic_np(np.zeros((4, 4), np.uint8), border='wrap')
    with pytest.raises(ValueError):
        robotcar.demosaic_np(np.zeros((1, 4), np.uint8))
    with pytest.raises(ValueError):
        robotcar.demosaic_np(np.zeros((4, 4), np.float32))


@pytest.mark.parametrize('sh,sw', D.SHAPES)
def test_the_statement_is_scipy_bit_for_bit(sh, sw):
    pytest.importorskip('scipy.ndimage')
    raw = D.raw_frames(2, sh, sw)
    luts = [D.mixed_lut(sh, sw, seed) for seed in range(5 if sh * sw <= 12 else 1)]
    for pattern in robotcar.PATTERNS:
        for border in robotcar.BORDERS:
            for frame in raw:
                want = _sdk_demosaic(frame, pattern, border)
                got = robotcar.demosaic_np(frame, pattern, border)
                assert got.dtype == np.float64 and got.shape == (sh, sw, 3)
                assert np.array_equal(got, want), (sh, sw, pattern, border)
                np.testing.assert_array_equal(robotcar.load_image_np(frame, pattern, None, border),
                                              want.astype(np.uint8))
                for lut in luts:
                    und = _sdk_undistort(want, lut)
                    mine = robotcar.undistort_np(got, lut)
                    assert not np.isnan(und).any()
                    assert np.array_equal(mine, und), (sh, sw, pattern, border)
                    np.testing.assert_array_equal(robotcar.load_image_np(frame, pattern, lut, border),
                                                  np.array(und).astype(np.uint8))


def test_reflect_wraps_at_the_border_and_mirror_does_not():
    raw = D.raw_frames(1, 6, 8)[0]
    assert raw.min() == 255
    q = robotcar.demosaic_np(raw, 'gbrg', 'reflect')
    assert q.max() == 573.75 and q[1:-1, 1:-1].max() == 255.0
    assert robotcar.load_image_np(raw, 'gbrg', None, 'reflect').min() == 573 - 512
    m = robotcar.demosaic_np(raw, 'gbrg', 'mirror')
    assert m.min() == 255.0 == m.max()
    for pattern in robotcar.PATTERNS:
        for frame in D.raw_frames(2, 7, 9):
            assert robotcar.demosaic_np(frame, pattern, 'mirror').max() <= 255.0


def test_the_mixed_table_holds_every_kind_of_coordinate():
    sh, sw = 96, 128
    lut = D.mixed_lut(sh, sw)
    ly, lx = lut[1], lut[0]
    assert np.isnan(ly).any() and np.isnan(lx).any()
    assert (ly == sh - 1).any() and (lx == sw - 1).any() and (ly == sh - 1 + 1e-12).any()
    assert (np.signbit(ly) & (ly == 0)).any() and ((ly == 0) & ~np.signbit(ly)).any()
    assert (ly < 0).any() and (ly > sh - 1).any() and (lx < 0).any() and (lx > sw - 1).any()
    assert (ly == np.rint(ly)).mean() > 0.2 and (ly != np.rint(ly)).mean() > 0.5


def test_an_identity_table_leaves_the_demosaic_unchanged():
    for sh, sw in ((2, 2), (7, 9), (96, 128)):
        raw = D.raw_frames(1, sh, sw)[0]
        ident = robotcar.identity_lut(sh, sw)
        assert ident.shape == (2, sh * sw) and ident.dtype == np.float64
        assert ident[0, 1] == 1.0 and ident[1, 1] == 0.0                      # columns first
        for border in robotcar.BORDERS:
            q = robotcar.demosaic_np(raw, 'gbrg', border)
            assert np.array_equal(robotcar.undistort_np(q, ident), q)
            np.testing.assert_array_equal(robotcar.load_image_np(raw, 'gbrg', ident, border),
                                          robotcar.load_image_np(raw, 'gbrg', None, border))


def test_table_file_round_trip_and_the_size_error(tmp_path):
    lut = D.mixed_lut(7, 9)
    path = tmp_path / 'stereo_narrow_left_distortion_lut.bin'
    robotcar.save_distortion_lut(lut, path)
    back = robotcar.load_distortion_lut(path, 7, 9)
    assert back.dtype == np.float64 and back.shape == (2, 63) and back.flags.c_contiguous
    np.testing.assert_array_equal(back, lut)                                  # NaN == NaN here
    with pytest.raises(ValueError, match='Incorrect image size for camera model'):
        robotcar.load_distortion_lut(path, 9, 9)
    with pytest.raises(ValueError, match='Incorrect image size for camera model'):
        robotcar.undistort_np(np.zeros((9, 9, 3)), lut)


# ---- the launcher ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_debayer_launcher_refuses_on_the_host(lib):
    from soft_contrastive_learning_amd import _lib
    NULL, SHAPE = -3, -1
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd, a4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 1), ctypes.c_void_p(base + 4)

    def call(raw=p, n=2, sh=8, sw=8, pattern=3, border=0, lut=p, xtab=p, ow=4, ytab=p, oh=4,
             kind=_lib.FRAMES_F32, out=p):
        return lib.scl_frames_debayer(raw, n, sh, sw, pattern, border, lut, xtab, ow, ytab, oh, kind, out, None)

    # NULL operands — before the shape (n = 0 is refused as a shape)
    assert call(raw=None, n=0) == NULL and call(out=None, n=0) == NULL
    assert call(xtab=None, n=0) == NULL and call(ytab=None, n=0) == NULL      # exactly one table
    assert call(n=0) == SHAPE and call(n=-1) == SHAPE and call(n=65536) == SHAPE
    assert call(sh=1) == SHAPE and call(sw=1) == SHAPE and call(sh=16385) == SHAPE and call(sw=16385) == SHAPE
    assert call(oh=0) == SHAPE and call(ow=0) == SHAPE and call(oh=16385) == SHAPE and call(ow=16385) == SHAPE
    assert call(pattern=4) == SHAPE and call(pattern=-1) == SHAPE
    assert call(border=2) == SHAPE and call(border=-1) == SHAPE
    assert call(kind=2) == SHAPE and call(kind=-1) == SHAPE
    assert call(out=odd) == SHAPE                                          # float32 at an odd address
    assert call(lut=a4) == SHAPE and call(lut=odd) == SHAPE                # float64 table, 8-byte aligned
    # without tables oh and ow are not read; a NULL table pair and a NULL lut are valid forms
    assert call(xtab=None, ytab=None, oh=0, ow=0, n=0) == SHAPE
    assert call(xtab=None, ytab=None, lut=None, n=0) == SHAPE
    assert call(out=odd, kind=_lib.FRAMES_U8, n=0) == SHAPE                # (bytes may sit there: n decides)
    assert lib.scl_abi_version() == 12
    assert _lib.SIGNATURES['scl_frames_debayer'][1][6] is ctypes.c_void_p


# ---- the command lines -----------------------------------------------------------------------------
def test_inference_refuses_bayer_without_device_resize(tmp_path):
    from soft_contrastive_learning_amd.evaluation import inference
    parser = inference.build_parser()
    f = parser.parse_args([])
    assert f.bayer == '' and f.distortion_lut == '' and f.bayer_border == 'reflect'
    lut = tmp_path / 'lut.bin'
    robotcar.save_distortion_lut(robotcar.identity_lut(4, 4), lut)
    common = ['--set', 'x', '--csv_root', str(tmp_path), '--img_root', str(tmp_path)]
    # each refusal comes before the model is made: no device is touched
    with pytest.raises(SystemExit, match='--device_resize 1'):
        inference.main(common + ['--bayer', 'gbrg', '--distortion_lut', str(lut)])
    with pytest.raises(SystemExit, match='--device_resize 1'):
        inference.main(common + ['--bayer', 'gbrg', '--distortion_lut', str(lut), '--device_resize', '0'])
    with pytest.raises(SystemExit, match='--distortion_lut'):
        inference.main(common + ['--bayer', 'gbrg', '--device_resize', '1'])
    with pytest.raises(SystemExit, match='--bayer'):
        inference.main(common + ['--distortion_lut', str(lut), '--device_resize', '1'])
    with pytest.raises(SystemExit, match='does not exist'):
        inference.main(common + ['--bayer', 'gbrg', '--distortion_lut', str(tmp_path / 'none.bin'),
                                 '--device_resize', '1'])
    with pytest.raises(SystemExit, match='CSV set'):
        inference.main(['--bayer', 'gbrg', '--distortion_lut', str(lut), '--device_resize', '1'])
    with pytest.raises(SystemExit):
        inference.main(common + ['--bayer', 'rgbg', '--distortion_lut', str(lut), '--device_resize', '1'])
    with pytest.raises(SystemExit):
        parser.parse_args(['--bayer_border', 'wrap'])


def test_raw_loader_wants_one_channel(tmp_path):
    from PIL import Image

    from soft_contrastive_learning_amd.evaluation import inference
    from soft_contrastive_learning_amd.util import io
    grey = D.raw_frames(1, 6, 8, seed=3)[0]
    Image.fromarray(grey).save(str(tmp_path / 'raw.png'))
    Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).save(str(tmp_path / 'rgb.png'))
    io.save_csv({'path': ['raw.png', 'rgb.png']}, str(tmp_path / 'cam.csv'))
    load, num = inference.csv_loader('cam', str(tmp_path), str(tmp_path), device_resize=True, bayer='gbrg')
    assert num == 2
    img, rule, kw = load(0)
    assert img.dtype == np.uint8 and img.shape == (6, 8) and (rule, kw) == ('resize_img', dict(max_size=240))
    np.testing.assert_array_equal(img, grey)
    with pytest.raises(ValueError, match='one 8-bit channel'):
        load(1)
    with pytest.raises(ValueError):
        inference.csv_loader('cam', str(tmp_path), str(tmp_path), device_resize=False, bayer='gbrg')


def test_robotcar_command_refuses_before_the_device(tmp_path):
    lut = tmp_path / 'lut.bin'
    robotcar.save_distortion_lut(robotcar.identity_lut(4, 4), lut)
    src = tmp_path / 'in'
    src.mkdir()
    good = ['--in_dir', str(src), '--out_dir', str(tmp_path / 'out'), '--distortion_lut', str(lut)]
    f = robotcar.build_parser().parse_args(good)
    assert (f.pattern, f.border, f.max_side, f.batch) == ('gbrg', 'reflect', 240, 16)
    with pytest.raises(SystemExit, match='no directory'):
        robotcar.main(['--in_dir', str(tmp_path / 'none')] + good[2:])
    with pytest.raises(SystemExit, match='does not exist'):
        robotcar.main(good[:4] + ['--distortion_lut', str(tmp_path / 'none.bin')])
    with pytest.raises(SystemExit, match='at least 1'):
        robotcar.main(good + ['--batch', '0'])
    with pytest.raises(SystemExit, match='at least 1'):
        robotcar.main(good + ['--max_side', '0'])
    with pytest.raises(SystemExit, match='overwritten'):
        robotcar.main(['--in_dir', str(src), '--out_dir', str(src), '--distortion_lut', str(lut)])
    with pytest.raises(SystemExit, match='no .png'):
        robotcar.main(good)
    with pytest.raises(SystemExit):
        robotcar.main(good + ['--pattern', 'rgbg'])
    assert not (tmp_path / 'out').exists()

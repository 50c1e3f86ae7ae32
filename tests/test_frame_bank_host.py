"""Host side of the frame bank (train/frame_bank.py): the slot bookkeeping, ``prepare`` against a
stub image set, the launcher's refusals and the uint8 loader of ``CsvImageSet`` — no GPU."""
import ctypes
import os

import numpy as np
import pytest

from soft_contrastive_learning_amd.train import frame_bank as FB


# ---- SlotMap ---------------------------------------------------------------------------------
def _adds_up(m):
    s = m.stats
    assert s['hits'] + s['decoded_positions'] == s['positions']
    assert s['decoded'] <= s['decoded_positions']


def test_duplicates_in_one_plan_are_decoded_once():
    m = FB.SlotMap(8)
    p = m.plan(['a', 'b', 'a', 'c', 'b', 'a'])
    assert p.decode == ['a', 'b', 'c']
    assert p.entries.tolist() == [-1, -2, -1, -3, -2, -1]
    assert p.owned == [(0, 0), (1, 1), (2, 2)]
    assert m.stats['decoded'] == 3 and m.stats['decoded_positions'] == 6 and m.stats['hits'] == 0
    _adds_up(m)


def test_only_committed_slots_hit_and_a_reserved_key_races():
    m = FB.SlotMap(8)
    first = m.plan(['a', 'b'])
    second = m.plan(['b', 'c', 'b'])              # b is reserved by `first`, not committed
    assert second.decode == ['b', 'c'] and second.entries.tolist() == [-1, -2, -1]
    assert second.owned == [(1, 2)]                  # c gets a slot, b travels as extra only
    assert m.stats['raced'] == 1 and m.stats['hits'] == 0
    m.commit(second)                                 # materialised in the OTHER order
    third = m.plan(['c', 'b', 'a'])
    assert third.entries.tolist() == [2, -1, -2] and m.stats['raced'] == 3
    m.commit(first)
    fourth = m.plan(['a', 'b', 'c', 'a'])
    assert fourth.entries.tolist() == [0, 1, 2, 0] and fourth.decode == [] and fourth.owned == []
    assert m.stats['hits'] == 5
    _adds_up(m)


def test_a_full_bank_bypasses():
    m = FB.SlotMap(2)
    p = m.plan(['a', 'b', 'c', 'd', 'c'])
    assert p.owned == [(0, 0), (1, 1)] and p.entries.tolist() == [-1, -2, -3, -4, -3]
    assert m.stats['bypassed'] == 2 and m.in_use == 2
    m.commit(p)
    q = m.plan(['c', 'a', 'e'])
    assert q.entries.tolist() == [-1, 0, -2] and q.owned == [] and m.stats['bypassed'] == 4
    _adds_up(m)


def test_capacity_zero_bypasses_everything():
    m = FB.SlotMap(0)
    for _ in range(2):
        p = m.plan(['a', 'b', 'a'])
        m.commit(p)
        assert p.owned == [] and p.entries.tolist() == [-1, -2, -1]
    assert m.stats['bypassed'] == 4 and m.stats['hits'] == 0 and m.in_use == 0
    _adds_up(m)


def test_a_released_plan_frees_its_slots_and_its_counts():
    m = FB.SlotMap(2)
    p = m.plan(['a', 'b'])
    m.release(p)
    assert m.in_use == 0 and all(v == 0 for v in m.stats.values())
    q = m.plan(['c', 'd', 'e'])
    assert sorted(s for _, s in q.owned) == [0, 1] and m.stats['bypassed'] == 1
    _adds_up(m)


# ---- FrameBank.prepare -----------------------------------------------------------------------
class StubSet:
    """Frames that are a function of the key; counts every decode."""

    def __init__(self, num=40, shape=(5, 7), other_shape_from=None):
        self.num, self.shape, self.other_shape_from = num, shape, other_shape_from
        self.decodes = []

    def __len__(self):
        return self.num

    def frame_key(self, i):
        return ('stub', int(i))

    def frame(self, i):
        h, w = self.shape if self.other_shape_from is None or i < self.other_shape_from else (3, 4)
        rng = np.random.default_rng(1000 + int(i))
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        f[0, 0, 0], f[0, 0, 1] = 0, 255
        return f

    def load_frames_u8(self, indices):
        self.decodes.extend(int(i) for i in indices)
        return np.stack([self.frame(i) for i in indices])

    def load_images(self, indices):
        return self.load_frames_u8(indices).astype(np.float32)


def test_prepare_plans_decodes_once_and_counts():
    s = StubSet()
    bank = FB.FrameBank(10 * 105, 'cuda:0')          # prepare() never touches the device
    p = bank.prepare(s, [3, 4, 3, 5])
    assert isinstance(p, FB.PendingFrames) and len(p) == 4
    assert bank.shape == (5, 7, 3) and bank.slots == 10
    assert s.decodes == [3, 4, 5] and p.new.dtype == np.uint8 and p.new.shape == (3, 5, 7, 3)
    assert p.plan.entries.tolist() == [-1, -2, -1, -3]
    for j, i in enumerate([3, 4, 5]):
        assert np.array_equal(p.new[j], s.frame(i))
    st = bank.stats
    assert st['decoded'] == 3 and st['hits'] == 0 and st['slots_in_use'] == 3 and st['bytes'] == 3 * 105
    assert st['hits'] + st['decoded_positions'] == st['positions'] == 4


def test_prepare_refuses_an_out_of_range_slot_entry():
    s = StubSet()
    bank = FB.FrameBank(10 * 105, 'cuda:0')
    bank.prepare(s, [0, 1])
    real = bank._map.plan

    def plan_with(entry):
        def plan(keys):
            p = real(keys)
            p.entries[-1] = entry
            return p
        return plan
    for entry in (10, 11, 2 ** 31 - 1, -3, -2 ** 31):     # the bank has 10 slots, the batch 2 new frames
        bank._map.plan = plan_with(entry)
        with pytest.raises(ValueError):
            bank.prepare(s, [2, 3])
    bank._map.plan = real
    assert bank.stats['slots_in_use'] == 2             # the refused plans gave their slots back
    for entry in (9, -2):                              # the last slot, the last new frame: inside
        bank._map.plan = plan_with(entry)
        bank.prepare(s, [4, 5])
    with pytest.raises(ValueError):
        FB.validate_entries([0], 0, 0)


def test_a_batch_of_another_shape_bypasses_the_bank():
    s = StubSet(other_shape_from=20)
    bank = FB.FrameBank(10 * 105, 'cuda:0')
    assert isinstance(bank.prepare(s, [0, 1]), FB.PendingFrames)
    before = bank.stats
    got = bank.prepare(s, [20, 21, 20])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (3, 3, 4, 3)
    assert np.array_equal(got, s.load_images([20, 21, 20]))
    after = bank.stats
    assert after['shape_bypassed'] == 1 and after['slots_in_use'] == before['slots_in_use'] == 2
    assert after['decoded'] == before['decoded']


def test_cached_image_set_presents_the_interface_of_the_loop():
    s = StubSet()
    s.xy, s.yaw = np.zeros((40, 2)), np.zeros(40)
    s.load_raw = lambda i: s.frame(i)
    c = FB.CachedImageSet(s, FB.FrameBank(1 << 20, 'cuda:0'))
    assert len(c) == 40 and c.xy is s.xy and c.yaw is s.yaw and c.num == 40
    assert np.array_equal(c.load_raw(3), s.frame(3))
    assert isinstance(c.load_images([1, 2]), FB.PendingFrames)
    assert FB.wrap(s, None) is s and isinstance(FB.wrap(s, c.bank), FB.CachedImageSet)
    plain = object()
    assert FB.wrap(plain, c.bank) is plain             # no frame_key: not wrapped


# ---- C-ABI refusals --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def test_gather_launcher_refuses_on_the_host(lib):
    NULL, SHAPE = -3, -1
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(bank=p, bank_slots=2, extra=p, extra_slots=2, slots=p, n=2, frame_bytes=48, out=p):
        return lib.scl_frames_gather(bank, bank_slots, extra, extra_slots, slots, n, frame_bytes, out, None)

    # NULL operands — before the shape (n = 0 is refused as a shape)
    assert call(out=None, n=0) == NULL and call(slots=None, n=0) == NULL
    assert call(bank=None, n=0) == NULL and call(extra=None, n=0) == NULL
    # shapes
    assert call(n=0) == SHAPE and call(n=-1) == SHAPE and call(n=65536) == SHAPE
    assert call(frame_bytes=0) == SHAPE and call(frame_bytes=-4) == SHAPE
    assert call(frame_bytes=2 ** 30 + 1) == SHAPE
    assert call(bank=None, bank_slots=0, extra=None, extra_slots=0) == SHAPE
    assert call(bank_slots=0, extra_slots=0) == SHAPE
    assert call(bank_slots=-1) == SHAPE and call(extra_slots=-1) == SHAPE
    assert call(bank_slots=2 ** 31) == SHAPE and call(extra_slots=2 ** 31) == SHAPE
    assert call(bank=None, bank_slots=-1) == SHAPE and call(extra=None, extra_slots=-1) == SHAPE
    assert lib.scl_abi_version() == 12


# ---- CsvImageSet -----------------------------------------------------------------------------
def _write_set(tmp_path):
    from soft_contrastive_learning_amd.util import io
    root = str(tmp_path / 'img')
    d = os.path.join(root, '2015-01-01-00-00-00_stereo_centre_01')
    os.makedirs(d)
    rng = np.random.default_rng(0)
    num = 5
    for i in range(num):
        io.save_img(rng.integers(0, 256, (30, 44, 3), dtype=np.uint8), os.path.join(d, '%d.png' % (100 + i)))
    cols = dict(date=['2015-01-01-00-00-00'] * num, folder=[1] * num, t=[100 + i for i in range(num)],
                easting=[float(i) for i in range(num)], northing=[0.0] * num, yaw=[0.0] * num)
    io.save_csv(cols, str(tmp_path / 'a.csv'))
    order = [3, 0, 4, 1, 2]
    io.save_csv({k: [v[i] for i in order] for k, v in cols.items()}, str(tmp_path / 'b.csv'))
    return root, order


@pytest.mark.parametrize('vlad_cores', [64, 0])
def test_csv_set_u8_frames_are_the_float_frames(tmp_path, vlad_cores):
    from soft_contrastive_learning_amd.train import dataset
    root, _ = _write_set(tmp_path)
    for threads in (1, 4):
        s = dataset.CsvImageSet(str(tmp_path / 'a.csv'), root, vlad_cores=vlad_cores, loader_threads=threads)
        idx = [4, 0, 2, 0]
        u8, f32 = s.load_frames_u8(idx), s.load_images(idx)
        assert u8.dtype == np.uint8 and f32.dtype == np.float32 and u8.shape == f32.shape
        assert u8.shape[0] == 4 and u8.shape[3] == 3
        assert np.array_equal(u8.astype(np.float32), f32)
        assert s.load_frames_u8([1]).shape == (1,) + u8.shape[1:]       # the single-frame route


def test_csv_set_frame_key_follows_the_file_and_the_sizing(tmp_path):
    from soft_contrastive_learning_amd.train import dataset
    root, order = _write_set(tmp_path)
    a = dataset.CsvImageSet(str(tmp_path / 'a.csv'), root)
    b = dataset.CsvImageSet(str(tmp_path / 'b.csv'), root)
    for pos, i in enumerate(order):
        assert b.frame_key(pos) == a.frame_key(i)
        assert hash(b.frame_key(pos)) == hash(a.frame_key(i))
    assert len({a.frame_key(i) for i in range(5)}) == 5
    c = dataset.CsvImageSet(str(tmp_path / 'a.csv'), root, vlad_cores=0)
    assert c.frame_key(0) != a.frame_key(0)
    assert dataset.CsvImageSet(str(tmp_path / 'a.csv'), root, max_side=120).frame_key(0) != a.frame_key(0)
    assert not hasattr(dataset.SyntheticImageSet(8), 'frame_key')

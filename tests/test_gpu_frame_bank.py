"""The frame bank on the device: scl_frames_gather against ``src.astype(np.float32)`` — EXACT
equality, every uint8 being a float32 —, FrameBank against a stub image set, and whole training
runs with and without ``--frame_cache_mb``, which must be equal record by record."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_frame_bank_host import StubSet

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


def _pixels(slots, frame_bytes, seed):
    a = np.random.default_rng(seed).integers(0, 256, (slots, frame_bytes), dtype=np.uint8)
    a[:, 0], a[:, -1] = 0, 255
    a[0, :2], a[-1, -2:] = (255, 0), (0, 255)
    return a


def _on_device(a, dev, offset):
    """The array on the device, starting ``offset`` bytes into its allocation."""
    raw = torch.zeros(a.size + offset, dtype=torch.uint8, device=dev)
    raw[offset:] = torch.from_numpy(a.reshape(-1)).to(dev)
    return raw[offset:].view(a.shape)


def _slot_list(n, bank_slots, extra_slots, rng):
    """Unsorted, with duplicates, the first and last frame of both sources."""
    pool = list(range(bank_slots)) + [-(j + 1) for j in range(extra_slots)]
    must = ([0, bank_slots - 1, 0] if bank_slots else []) + ([-1, -extra_slots, -extra_slots] if extra_slots else [])
    s = must + [pool[i] for i in rng.integers(0, len(pool), max(n - len(must), 0))]
    s = [s[i] for i in rng.permutation(len(s))]
    return s[:n]


def _gather(lib, dev, bank, bank_np, extra, extra_np, slots, frame_bytes, out_offset=0):
    """Run the kernel; check the result, the sentinels around it and the sources."""
    from soft_contrastive_learning_amd import _lib
    n = len(slots)
    flat = torch.full((out_offset + (n + 1) * frame_bytes,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[out_offset:]
    st = torch.tensor(slots, dtype=torch.int32, device=dev)
    code = lib.scl_frames_gather(_lib.ptr(bank), 0 if bank is None else bank.shape[0],
                                 _lib.ptr(extra), 0 if extra is None else extra.shape[0],
                                 _lib.ptr(st), n, frame_bytes, _lib.ptr(out), _lib.stream_of(out))
    assert code == 0
    got = flat.cpu().numpy()
    want = np.stack([bank_np[s] if s >= 0 else extra_np[-s - 1] for s in slots]).astype(np.float32)
    assert np.array_equal(got[out_offset:out_offset + n * frame_bytes].reshape(n, frame_bytes), want)
    assert (got[:out_offset] == SENTINEL).all() and (got[out_offset + n * frame_bytes:] == SENTINEL).all()
    if bank is not None:
        assert np.array_equal(bank.cpu().numpy(), bank_np)
    if extra is not None:
        assert np.array_equal(extra.cpu().numpy(), extra_np)


# (H, W), the batch sizes
SHAPES = [((4, 4), (1, 70)),            # 48 bytes: a multiple of 16
          ((6, 10), (1, 70)),           # 180: a multiple of 4, not of 16
          ((5, 7), (1, 70)),            # 105: odd source offsets, output frames only 4-byte aligned
          ((180, 240), (1, 25, 70)),    # the training shape
          ((480, 640), (1, 3, 70))]     # the bench shape


@pytest.mark.parametrize("hw,sizes", SHAPES, ids=["%dx%d" % s[0] for s in SHAPES])
def test_gather_is_exact_at_every_alignment(lib, dev, hw, sizes):
    frame_bytes = hw[0] * hw[1] * 3
    bank_slots, extra_slots = 13, 5
    bank_np, extra_np = _pixels(bank_slots, frame_bytes, 1), _pixels(extra_slots, frame_bytes, 2)
    rng = np.random.default_rng(frame_bytes)
    bank, extra = _on_device(bank_np, dev, 0), _on_device(extra_np, dev, 0)
    bank1, extra3 = _on_device(bank_np, dev, 1), _on_device(extra_np, dev, 3)   # views at a byte offset
    assert bank1.data_ptr() % 2 == 1 and extra3.data_ptr() % 4 == 3
    for n in sizes:
        if n == 1:
            lists = [[0], [bank_slots - 1], [-1], [-extra_slots]]
            only_bank, only_extra = [[0], [bank_slots - 1]], [[-1], [-extra_slots]]
        elif n == 3:
            lists = [[bank_slots - 1, -extra_slots, 0], [-1, 0, -1]]
            only_bank, only_extra = [[bank_slots - 1, 0, 0]], [[-extra_slots, -1, -extra_slots]]
        else:
            lists = [_slot_list(n, bank_slots, extra_slots, rng)]
            assert len(set(lists[0])) < n and sorted(lists[0]) != lists[0]
            assert {0, bank_slots - 1, -1, -extra_slots} <= set(lists[0])
            some = lists[0][:23]          # (the one-source calls need not be the largest)
            only_bank = [[abs(s) % bank_slots for s in some] + [bank_slots - 1, 0]]
            only_extra = [[-(abs(s) % extra_slots) - 1 for s in some] + [-extra_slots, -1]]
        for slots in lists:
            _gather(lib, dev, bank, bank_np, extra, extra_np, slots, frame_bytes)
            _gather(lib, dev, bank1, bank_np, extra3, extra_np, slots, frame_bytes)
        # one source only: extra NULL / bank NULL with no slots
        for slots in only_bank:
            _gather(lib, dev, bank, bank_np, None, None, slots, frame_bytes)
            _gather(lib, dev, bank1, bank_np, None, None, slots, frame_bytes)
        for slots in only_extra:
            _gather(lib, dev, None, None, extra, extra_np, slots, frame_bytes)
    # an output that is 4-byte but not 16-byte aligned: a head in front of every frame's float4 body
    n = sizes[1]
    _gather(lib, dev, bank1, bank_np, extra, extra_np, _slot_list(n, bank_slots, extra_slots, rng),
            frame_bytes, out_offset=1)
    _gather(lib, dev, bank, bank_np, extra3, extra_np, _slot_list(n, bank_slots, extra_slots, rng),
            frame_bytes, out_offset=3)


def _want(s, indices):
    return np.stack([s.frame(i) for i in indices]).astype(np.float32)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_plans_sharing_new_frames_materialise_in_either_order(dev, order):
    """The depth-2 pipeline's situation: the second batch is prepared before the first one is on
    the device."""
    from soft_contrastive_learning_amd.train import frame_bank as FB
    s = StubSet()
    bank = FB.FrameBank(1 << 20, dev)
    idx = ([0, 1, 2, 3, 1], [2, 3, 4, 5, 2, 0])
    pend = [bank.prepare(s, idx[0]), bank.prepare(s, idx[1])]
    assert bank.stats['raced'] == 3                    # 2, 3 and 0 were reserved, not committed
    for k in order:
        out = FB.to_device(pend[k], dev)
        assert out.dtype == torch.float32 and out.shape == (len(idx[k]), 5, 7, 3) and out.is_cuda
        assert np.array_equal(out.cpu().numpy(), _want(s, idx[k]))
    decodes = len(s.decodes)
    again = [5, 4, 3, 2, 1, 0, 5]
    p = bank.prepare(s, again)
    assert p.new is None and len(s.decodes) == decodes and (p.plan.entries >= 0).all()
    assert np.array_equal(FB.to_device(p, dev).cpu().numpy(), _want(s, again))
    st = bank.stats
    assert st['hits'] == 7 and st['slots_in_use'] == 6 and st['hits'] + st['decoded_positions'] == st['positions']


def test_a_full_bank_serves_the_rest_from_the_batch(dev):
    from soft_contrastive_learning_amd.train import frame_bank as FB
    s = StubSet()
    bank = FB.FrameBank(10 * 105 + 50, dev)            # 10 slots of 5 x 7 x 3
    for _ in range(2):
        for start in range(0, 25, 7):
            idx = list(range(start, min(start + 7, 25))) + [start, 24 - start]
            assert np.array_equal(FB.to_device(bank.prepare(s, idx), dev).cpu().numpy(), _want(s, idx))
    st = bank.stats
    assert bank.slots == 10 and st['slots_in_use'] == 10 and st['bypassed'] > 0 and st['hits'] > 0
    assert st['bytes'] == 10 * 105


def test_a_second_pass_decodes_nothing_and_another_stream_is_refused(dev):
    from soft_contrastive_learning_amd.train import frame_bank as FB
    s = StubSet(num=30, shape=(6, 10))
    bank = FB.FrameBank(1 << 20, dev)
    batches = [list(range(k, k + 10)) for k in (0, 10, 20)]
    for idx in batches:
        FB.to_device(bank.prepare(s, idx), dev)
    assert sorted(s.decodes) == list(range(30)) and bank.stats['decoded'] == 30
    for idx in batches[::-1]:
        assert np.array_equal(FB.to_device(bank.prepare(s, idx[::-1]), dev).cpu().numpy(), _want(s, idx[::-1]))
    assert len(s.decodes) == 30 and bank.stats['decoded'] == 30 and bank.stats['hits'] == 30
    # a float32 host batch (a set without frame keys) goes up as before
    host = s.load_images([1, 2])
    assert np.array_equal(FB.to_device(host, dev).cpu().numpy(), host)
    p = bank.prepare(s, [0, 1])
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        with pytest.raises(RuntimeError):
            bank.materialize(p)
    assert np.array_equal(bank.materialize(p).cpu().numpy(), _want(s, [0, 1]))


def _write_lists(tmp_path):
    """Per-epoch lists 000 and 001 over the same PNG files in different orders, the thinned
    localisation references, in the reference's layout."""
    from soft_contrastive_learning_amd.train import dataset
    from soft_contrastive_learning_amd.util import io
    img_root, lists = str(tmp_path / 'img'), tmp_path / 'lists'
    lists.mkdir()
    for name, num, seed, folder in (('train_ref', 32, 1, 1), ('train_query', 32, 101, 2),
                                    ('test_ref', 32, 3, 3), ('test_query', 32, 103, 4)):
        # two laps of a 420 m loop: every anchor has a positive (its place on the other lap) and
        # twelve negatives that are 15 m from it and from each other
        syn = dataset.SyntheticImageSet(num, 48, 64, spacing=420.0 / (num // 2), seed=seed, distractor=0.3)
        frames = syn.load_images(np.arange(num)).clip(0, 255).astype(np.uint8)
        d = os.path.join(img_root, '2015-01-01-00-00-00_stereo_centre_{:02d}'.format(folder))
        os.makedirs(d)
        for i in range(num):
            io.save_img(frames[i], os.path.join(d, '%d.png' % (1000 + i)))
        cols = dict(date=['2015-01-01-00-00-00'] * num, folder=[folder] * num, t=[1000 + i for i in range(num)],
                    easting=[float(v) for v in syn.xy[:, 0]], northing=[float(v) for v in syn.xy[:, 1]],
                    yaw=[float(v) for v in syn.yaw])
        io.save_csv(cols, str(lists / ('%s_000.csv' % name)))
        order = np.random.RandomState(folder).permutation(num)
        io.save_csv({k: [v[i] for i in order] for k, v in cols.items()}, str(lists / ('%s_001.csv' % name)))
        if 'ref' in name:
            keep = list(range(0, num, 2))
            io.save_csv({k: [cols[k][i] for i in keep] for k in cols if k != 'yaw'},
                        str(lists / ('%s_2.csv' % name)))
    return img_root, str(lists)


def test_training_runs_are_equal_with_and_without_the_frame_bank(dev, tmp_path, monkeypatch):
    """Three runs of two epochs on PNG files, mining and evaluation firing in both: without the bank,
    with an ample one and with one of ten frames.  Every step's loss and every evaluation record
    must be EQUAL; with the ample bank every file is decoded exactly once in the run.

    The tuples have the reference's 25 images: every pass of the run then has enough tiles for the
    project's own convolution kernels (nets._lds_conv_pays), which are bit-reproducible.  Measured
    while this test was written: at 7-image tuples conv4_x / conv5_x go to the library and two
    UNCACHED runs of this trainer already differ in the last digits of their losses (1.5860923 /
    1.5860936 at step 2); at 25 images two uncached runs are equal."""
    from soft_contrastive_learning_amd.train import dataset, train as T
    img_root, lists = _write_lists(tmp_path)
    decoded, real = [], dataset.load_frame

    def counting(path, *a, **kw):
        decoded.append(path)
        return real(path, *a, **kw)
    monkeypatch.setattr(dataset, 'load_frame', counting)

    def run(name, *extra):
        del decoded[:]
        out = str(tmp_path / 'out')
        # the mining cache covers the whole training list: every frame the pipeline's worker thread
        # asks for has been committed by the first refresh, so the ample bank never decodes twice
        state = T.main(['--loss', 'wms', '--shuffled_root', lists, '--img_root', img_root,
                        '--loc_ref_root', lists, '--positives_per_tuple', '12', '--negatives_per_tuple', '12',
                        '--hard_positives_per_tuple', '6', '--hard_negatives_per_tuple', '6',
                        '--mining_step', '3', '--mining_cache_size', '32', '--eval_step', '3',
                        '--save_step', '100', '--num_eval_queries', '6', '--eval_ref_r', '2',
                        '--steps', '4', '--max_epoch', '2', '--base_lr', '1e-5', '--dtype', 'bf16',
                        '--save_examples', '0', '--tensorboard', '0',
                        '--out_root', out, '--out_folder', name] + list(extra))
        recs = [json.loads(l) for l in open(os.path.join(out, name, 'train_log.txt'))]
        return state, recs, list(decoded)

    def outcome(recs):
        steps = [(r['step'], r['epoch'], r['loss']) for r in recs if 'loss' in r]
        evals = [(r['step'], r['other_region_loss'], r['other'], r['local'])
                 for r in recs if r.get('event') == 'eval']
        return steps, evals

    _, plain, plain_files = run('plain')
    state_a, ample, ample_files = run('ample', '--frame_cache_mb', '64')
    state_t, tight, tight_files = run('tight', '--frame_cache_mb', '1.24')    # 10 frames of 180 x 240 x 3
    steps, evals = outcome(plain)
    assert len(steps) >= 6 and {e for _, e, _ in steps} == {0, 1} and all(np.isfinite(l) for _, _, l in steps)
    assert len(evals) == 4 and len([r for r in plain if r.get('event') == 'mining_cache']) == 4
    assert not any('frame_bank' in r for r in plain)
    assert outcome(ample) == (steps, evals)
    assert outcome(tight) == (steps, evals)
    # the ample bank: one decode per distinct file of the run; the second epoch decodes only files
    # the first never touched
    st = state_a['frame_bank_stats']
    assert st['decoded'] == len(ample_files) == len(set(ample_files)) and set(ample_files) == set(plain_files)
    assert st['slots_in_use'] == st['decoded'] and st['bypassed'] == 0 and st['hits'] > st['decoded']
    assert st['hits'] + st['decoded_positions'] == st['positions']
    epochs = [r for r in ample if r.get('event') == 'epoch']
    assert [r['frame_bank']['decoded'] for r in epochs][0] == 0
    first = epochs[1]['frame_bank']['decoded']
    assert 0 < first <= len(ample_files) and not set(ample_files[first:]) & set(ample_files[:first])
    assert len(plain_files) > len(set(plain_files))              # the uncached run decodes files again
    # the bank of ten frames
    st = state_t['frame_bank_stats']
    assert st['slots'] == 10 and st['slots_in_use'] == 10 and st['bypassed'] > 0 and st['hits'] > 0
    assert len(set(tight_files)) == len(set(plain_files)) and len(tight_files) < len(plain_files)

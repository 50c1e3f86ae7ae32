"""Measures the device-resident frame bank (train/frame_bank.py, csrc/frames.hip) on the MI355X.

Part 1, the kernel.  ``scl_frames_gather`` assembling a float32 batch from a uint8 bank, at the
trainer's batch (25 x 180 x 240 x 3) and the bench's (24 x 480 x 640 x 3); all slots are bank
hits in random order — the steady state.  Beside it, in the same run:

* what it replaces in the loop: ``torch.from_numpy(float32 batch).to(dev)`` of the same batch
  (pageable host memory, host clock around the call + synchronise);
* ``FrameBank.materialize`` of an all-hits batch: the kernel plus the upload of the slot list and
  the allocation of the output, as the loop calls it;
* a device ``copy_`` of a float32 tensor of the output's size: the streaming rate of the same
  device for the same number of bytes written (it reads 4 bytes per value, the gather 1), against
  which the kernel's GB/s is read.

Medians of --reps calls after a warm-up, HIP events around each call.  Bytes of the gather:
n * frame_bytes read + 4 * n * frame_bytes written.

Part 2, the loop.  Writes --frames synthetic 1280 x 960 PNGs and per-epoch lists to a temporary
directory and, after a short warm-up run, runs the trainer for two epochs without and with
``--frame_cache_mb``, same arguments (25-image tuples), same process.  Per epoch: seconds per training step, per mining-cache refresh and per
evaluation (the time from the previous log record to the record of the event), and the epoch's
wall time; the losses of both runs are compared.

    python scripts/frame_cache_bench.py [--reps 50] [--frames 320] [--steps 20] [--skip_loop] [--json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from soft_contrastive_learning_amd import _lib as L  # noqa: E402
from soft_contrastive_learning_amd.train import frame_bank as FB  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def event_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return median(a.elapsed_time(b) * 1e3 for a, b in ev)


def host_us(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return median(t)


class ArraySet:
    """uint8 frames in memory behind the interface FrameBank.prepare takes."""

    def __init__(self, frames):
        self.frames = frames

    def frame_key(self, i):
        return int(i)

    def load_frames_u8(self, indices):
        return self.frames[list(indices)]


def kernel_part(dev, reps):
    lib, out = L.load(), []
    for n, h, w in ((25, 180, 240), (24, 480, 640)):
        fb = h * w * 3
        slots_n = 4 * n
        rng = np.random.default_rng(n)
        frames = rng.integers(0, 256, (slots_n, h, w, 3), dtype=np.uint8)
        bank = torch.from_numpy(frames).to(dev)
        pick = rng.permutation(slots_n)[:n].astype(np.int32)
        slots = torch.from_numpy(pick).to(dev)
        res = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
        stream = L.stream_of(res)

        def gather():
            L.check(lib.scl_frames_gather(L.ptr(bank), slots_n, None, 0, L.ptr(slots), n, fb, L.ptr(res), stream))
        gather()
        host_batch = frames[pick].astype(np.float32)
        assert np.array_equal(res.cpu().numpy(), host_batch)
        src = torch.from_numpy(host_batch).to(dev)
        dst = torch.empty_like(src)
        fbank = FB.FrameBank(slots_n * fb, dev)
        aset = ArraySet(frames)
        fbank.materialize(fbank.prepare(aset, range(slots_n)))
        pending = fbank.prepare(aset, pick)
        assert pending.new is None
        rec = dict(part='kernel', n=n, height=h, width=w, frame_bytes=fb,
                   gather_us=event_us(gather, reps),
                   materialize_hits_us=host_us(lambda: fbank.materialize(pending), reps),
                   host_float32_upload_us=host_us(lambda: torch.from_numpy(host_batch).to(dev), reps),
                   device_copy_us=event_us(lambda: dst.copy_(src), reps))
        rec['gather_bytes'] = 5 * n * fb
        rec['gather_GBps'] = rec['gather_bytes'] / rec['gather_us'] / 1e3
        rec['device_copy_GBps'] = 8 * n * fb / rec['device_copy_us'] / 1e3
        rec['device_copy_written_GBps'] = 4 * n * fb / rec['device_copy_us'] / 1e3
        rec['gather_written_GBps'] = 4 * n * fb / rec['gather_us'] / 1e3
        out.append(rec)
        print('%2d x %3d x %3d x 3: gather %8.1f us (%6.1f GB/s moved, %6.1f GB/s written) | materialize, all hits '
              '%8.1f us | float32 upload from the host %9.1f us | device copy_ of the output %8.1f us '
              '(%6.1f GB/s moved, %6.1f GB/s written)'
              % (n, h, w, rec['gather_us'], rec['gather_GBps'], rec['gather_written_GBps'],
                 rec['materialize_hits_us'], rec['host_float32_upload_us'], rec['device_copy_us'],
                 rec['device_copy_GBps'], rec['device_copy_written_GBps']))
        fbank.close()
    return out


def write_dataset(root, frames):
    """--frames PNGs of 1280 x 960 in the reference's layout, the lists of epochs 000 and 001."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from soft_contrastive_learning_amd.train import dataset
    from soft_contrastive_learning_amd.util import io
    img_root, lists = os.path.join(root, 'img'), os.path.join(root, 'lists')
    os.makedirs(lists)
    share = {'train_ref': 0.4, 'train_query': 0.2, 'test_ref': 0.2, 'test_query': 0.2}
    with ThreadPoolExecutor(16) as pool:
        for folder, (name, part) in enumerate(share.items(), 1):
            num = max(int(frames * part), 30)
            # two laps of a 480 m loop whatever the count: room for 12 negatives that are 15 m from
            # the anchor and from each other
            syn = dataset.SyntheticImageSet(num, 960, 1280, spacing=480.0 / (num // 2), seed=folder,
                                            distractor=0.3)
            d = os.path.join(img_root, '2015-01-01-00-00-00_stereo_centre_{:02d}'.format(folder))
            os.makedirs(d)

            def one(i, syn=syn, d=d):
                px = syn.load_images([i])[0].clip(0, 255).astype(np.uint8)
                Image.fromarray(px).save(os.path.join(d, '%d.png' % (1000 + i)), compress_level=1)
            list(pool.map(one, range(num)))
            cols = dict(date=['2015-01-01-00-00-00'] * num, folder=[folder] * num,
                        t=[1000 + i for i in range(num)], easting=[float(v) for v in syn.xy[:, 0]],
                        northing=[float(v) for v in syn.xy[:, 1]], yaw=[float(v) for v in syn.yaw])
            io.save_csv(cols, os.path.join(lists, '%s_000.csv' % name))
            order = np.random.RandomState(folder).permutation(num)
            io.save_csv({k: [v[i] for i in order] for k, v in cols.items()},
                        os.path.join(lists, '%s_001.csv' % name))
    return img_root, lists


def loop_part(f):
    from soft_contrastive_learning_amd.train import train as T
    out = []
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        img_root, lists = write_dataset(root, f.frames)
        print('wrote the PNG files in %.1f s' % (time.perf_counter() - t0))
        stamps = []
        real = T.train_dataset_epoch

        def stamped(flags, epoch, state, log):
            def log2(rec):
                stamps.append((time.perf_counter(), rec))
                log(rec)
            real(flags, epoch, state, log2)
            torch.cuda.synchronize()
            stamps.append((time.perf_counter(), {'event': 'epoch_end', 'epoch': epoch}))
        T.train_dataset_epoch = stamped
        try:
            losses = {}

            def run(name, epochs, steps, extra):
                # the reference's tuple, 25 images: every pass then runs on the project's own,
                # bit-reproducible convolution kernels and the two runs can be compared exactly
                return T.main(['--loss', 'wms', '--shuffled_root', lists, '--img_root', img_root,
                               '--positives_per_tuple', '12', '--negatives_per_tuple', '12',
                               '--hard_positives_per_tuple', '6', '--hard_negatives_per_tuple', '6',
                               '--mining_step', str(f.mining_step), '--mining_cache_size', str(f.mining_cache_size),
                               '--eval_step', str(f.eval_step), '--save_step', '100000',
                               '--num_eval_queries', '10', '--eval_ref_r', '2', '--steps', str(steps),
                               '--max_epoch', str(epochs), '--dtype', 'bf16', '--save_examples', '0',
                               '--tensorboard', '0', '--out_root', os.path.join(root, 'out'),
                               '--out_folder', name] + extra)
            run('warmup', 1, 2, [])            # code objects, first launches, the checkpoint writer
            for name, extra in (('uncached', []), ('cached', ['--frame_cache_mb', str(f.frame_cache_mb)])):
                del stamps[:]
                state = run(name, 2, f.steps, extra)
                losses[name] = [r['loss'] for _, r in stamps if 'loss' in r]
                # a record's time is the time since the record before it: a step's includes the wait for
                # its batch, a refresh or an evaluation is one record
                per = {e: {'step': [], 'mining_cache': [], 'eval': []} for e in (0, 1)}
                begin, end, prev, cur = {}, {}, None, None
                for t, r in stamps:
                    ev = r.get('event')
                    if ev == 'epoch':
                        cur = r['epoch']
                        begin[cur] = t
                    elif ev == 'epoch_end':
                        end[r['epoch']] = t
                    elif ev in ('mining_cache', 'eval'):
                        per[cur][ev].append(t - prev)
                    elif 'loss' in r:
                        per[cur]['step'].append(t - prev)
                    prev = t
                for epoch in (0, 1):
                    kinds = per[epoch]
                    rec = dict(part='loop', run=name, epoch=epoch, steps=len(kinds['step']),
                               step_s_median=median(kinds['step']), step_s_mean=float(np.mean(kinds['step'])),
                               mining_events=len(kinds['mining_cache']),
                               mining_s_mean=float(np.mean(kinds['mining_cache'])),
                               eval_events=len(kinds['eval']), eval_s_mean=float(np.mean(kinds['eval'])),
                               epoch_s=end[epoch] - begin[epoch])
                    if name == 'cached' and epoch == 1:
                        rec['frame_bank'] = state['frame_bank_stats']
                    out.append(rec)
                    print('%-8s epoch %d: %2d steps, %.4f s per step (median; mean %.4f) | %d mining refreshes, '
                          '%.3f s each | %d evaluations, %.3f s each | epoch %.2f s'
                          % (name, epoch, rec['steps'], rec['step_s_median'], rec['step_s_mean'],
                             rec['mining_events'], rec['mining_s_mean'], rec['eval_events'], rec['eval_s_mean'],
                             rec['epoch_s']))
            same = losses['uncached'] == losses['cached']
            print('losses of the two runs equal: %s (%d steps)' % (same, len(losses['cached'])))
            print('frame bank at the end of the cached run: %s' % json.dumps(state['frame_bank_stats']))
            out.append(dict(part='loop', losses_equal=same, steps=len(losses['cached'])))
        finally:
            T.train_dataset_epoch = real
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=50)
    p.add_argument('--frames', type=int, default=320, help='PNG files of the loop part')
    p.add_argument('--steps', type=int, default=20, help='training steps per epoch of the loop part')
    p.add_argument('--mining_step', type=int, default=10)
    p.add_argument('--mining_cache_size', type=int, default=50)
    p.add_argument('--eval_step', type=int, default=10)
    p.add_argument('--frame_cache_mb', type=float, default=256.0)
    p.add_argument('--skip_loop', action='store_true')
    p.add_argument('--json', action='store_true')
    f = p.parse_args(argv)
    assert torch.cuda.is_available(), 'frame_cache_bench.py measures on a HIP device'
    dev = torch.device('cuda:0')
    prop = torch.cuda.get_device_properties(dev)
    print('box: %s (%s), %d CUs, %.0f GB; torch %s, HIP %s; %d host cores seen'
          % (prop.name, getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count,
             prop.total_memory / 1e9, torch.__version__, torch.version.hip, os.cpu_count()))
    out = kernel_part(dev, f.reps)
    if not f.skip_loop:
        out += loop_part(f)
    if f.json:
        for rec in out:
            print(json.dumps(rec))


if __name__ == '__main__':
    main()

"""Trainer counterpart of the reference's ``train/train.py`` for the hot path.

Keeps the reference's flag names and defaults (train/train.py:1226-1312), the loss
dispatch of ``build_model`` (:585-879), the tuple/batch layout (``[anchor, P positives,
N negatives(, other negative)]`` per tuple, :502-503, 561, 589-594, 654), the learning-rate
schedule (:118-121), the optimisers (:865-878) and the three checkpoint cadences
(:935-937, 1070-1102).  Two data routes:

* ``--synthetic_dataset M`` or ``--shuffled_root DIR`` (+ ``--img_root``): the reference's
  epoch loop (``train_one_epoch`` :987-1109) on a pose-tagged image set — anchors go through
  ``TupleSampler`` -> ``InputPipeline`` (a worker thread samples tuples and loads images while
  the device trains, :226-260); every ``mining_step`` anchors the descriptors of
  ``mining_cache_size`` images plus the next anchors are cached for hard-negative mining
  (``MiningCache``, :1014-1068); every ``eval_step`` anchors a rolling checkpoint is written,
  the loss on the other region is measured (``get_eval_loss`` :1112-1149) and localisation is
  evaluated on both regions with the exact HIP top-5 (``evaluate_localization`` :1156-1193);
  every ``save_step`` a part checkpoint (:1094-1102).
* default: ``SyntheticTuples`` — random images with the per-loss ``distances`` payload the GPU
  thread receives (:263-275); what bench.py's workload looks like.

``--frame_cache_mb MB`` (default 0: off) keeps every frame of the ``--shuffled_root`` sets on the
device as the uint8 pixels the loader produced and assembles every batch — training, mining
refresh, evaluation — there with one HIP kernel (train/frame_bank.py, csrc/frames.hip): a file
is decoded, resized and uploaded once per run instead of once per use.  The batches are the same
float32 values bit for bit; each ``epoch`` record of the log then carries the bank's counters.
One bank per process (per rank), fill-only: frames beyond the capacity travel with their batch.

``--optimizer_impl hip`` (default ``torch``) takes the parameter update from this package's own
kernel instead of torch's fused one (train/optim.py HipAdam / HipMomentum, csrc/optim.hip): one
launch over every parameter, TensorFlow's float32 sequence bit for bit, the two beta powers
float32 accumulators on the device, which the checkpoints then store as they are.  Float32
parameters only.  With it, ``--skip_nonfinite 1`` runs one pass over the flat gradient buffer
before the update (scl_grad_stats) and hands its flag to the kernel: a step whose gradients hold
a NaN or an infinity changes no weight, no slot and not the step count, and says so in one line;
every step record then carries ``grad_norm`` and ``skipped``.

Of the eigenvalue and residual-determinant families wrd, prodwrd, sumwrd, residual_trace,
ntuplet_evmm, ntuplet_trace and ms_sum train here (model/losses.py).  Still refused:

* ``--loss residual_det``, ``--loss swrd`` and the sampler's ``'swrd'`` payload: the loss functions
  exist (``residual_det_loss``, ``swrd_loss``) and ms_sum trains through the first, but the two
  names are not switched on in the trainer yet;
* ``pairwise_distance_neg_eigenvalue`` and ``pairwise_huber_distance_neg_eigenvalue``: the
  reference trains them with two ``optimizer.minimize`` calls per batch (PN_LOSS, :872-875), which
  changes the training step; ``neg_eigenvalue_loss`` is the part of them that exists;
* the ``incremental_*`` losses and ``ms_det``: stateful incremental PCA (and its PCA threads,
  SURVEY.md §2).

    python -m soft_contrastive_learning_amd.train.train --loss wms --vlad_cores 64 \
        --reduction none --tuples_per_batch 1 --steps 20
    python -m soft_contrastive_learning_amd.train.train --loss wms --synthetic_dataset 400 \
        --height 64 --width 80 --positives_per_tuple 4 --negatives_per_tuple 4
    python -m torch.distributed.run --nproc-per-node 8 -m soft_contrastive_learning_amd.train.train ...
"""
import argparse
import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from .. import checkpoint, parallel, pointnetvlad_cls
from ..model import losses, nets, reduction
from .optim import GradStats, make_optimizer


def make_parser():
    p = argparse.ArgumentParser()
    # output / restore (train/train.py:1233-1238)
    p.add_argument('--checkpoint', default='')
    p.add_argument('--resume', action='store_true',
                   help='also restore the optimizer slots and the global step from --checkpoint '
                        '(the reference only warm-starts the weights, train/train.py:882-905)')
    p.add_argument('--out_root', default='./scl_logs')
    p.add_argument('--out_folder', default='')
    p.add_argument('--max_to_keep', type=int, default=1)
    # tuple size (:1241-1249)
    p.add_argument('--positives_per_tuple', type=int, default=12)
    p.add_argument('--negatives_per_tuple', type=int, default=12)
    p.add_argument('--hard_negatives_per_tuple', type=int, default=6)
    p.add_argument('--hard_positives_per_tuple', type=int, default=6)
    p.add_argument('--mutually_exclusive_negs', type=bool, default=True)
    # loss (:1252-1266)
    p.add_argument('--loss', default='wms')
    p.add_argument('--margin_1', type=float, default=0.1)
    p.add_argument('--margin_2', type=float, default=0.2)
    p.add_argument('--alpha', type=float, default=0.8)
    p.add_argument('--beta', type=float, default=15)
    p.add_argument('--wfunction', default='exp', help='exp, lin, tanh')
    p.add_argument('--sumfunction', default='ms', help='ms, plain')
    p.add_argument('--msmining', type=bool, default=False)   # type=bool as in the reference
    p.add_argument('--lam', type=float, default=0.5, help='Scaling factor between loss components.')
    p.add_argument('--max_pos_radius', type=float, default=15)
    p.add_argument('--min_neg_radius', type=float, default=15)
    # training (:1269-1281)
    p.add_argument('--tuples_per_batch', type=int, default=1)
    p.add_argument('--max_epoch', type=int, default=5)
    p.add_argument('--base_lr', type=float, default=5e-6)
    p.add_argument('--minimal_lr', type=float, default=5e-12)
    p.add_argument('--lr_down_factor', type=float, default=0.5)
    p.add_argument('--lr_down_frequency', type=float, default=1)
    p.add_argument('--momentum', type=float, default=0.9)
    p.add_argument('--optimizer', default='adam', help='adam, momentum')
    p.add_argument('--optimizer_impl', default='torch', choices=['torch', 'hip'],
                   help="torch: the update on torch's fused kernels (TFAdam / SGD); hip: this package's "
                        'update kernel, TensorFlow\'s float32 sequence bit for bit (train/optim.py)')
    p.add_argument('--skip_nonfinite', type=int, default=0,
                   help='1 (needs --optimizer_impl hip): a step whose gradients hold a NaN or an infinity '
                        'changes nothing; every step record carries grad_norm and skipped')
    # head (:1283-1289): none, or a dense reduction head 1fc|2fc|3fc of --out_dim units
    # (model/reduction.py); spp and the training-time pca need reference modules that do not exist
    p.add_argument('--out_dim', default=512, type=int)
    p.add_argument('--reduction', default='none', help='none, 1fc, 2fc, 3fc')
    p.add_argument('--vlad_cores', default=64, type=int)
    # the NetVLAD head from data (model/vlad_init.py; new work: the reference warm-starts from a
    # released model that has one)
    p.add_argument('--vlad_init', default='none', choices=['none', 'kmeans'],
                   help='kmeans: before the first step, seed the NetVLAD head with k-means on conv5_3 '
                        'descriptors of --vlad_init_images frames of the training set; --checkpoint may '
                        'then lack the two head variables')
    p.add_argument('--vlad_init_images', type=int, default=500)
    p.add_argument('--vlad_init_per_image', type=int, default=100)
    p.add_argument('--vlad_init_iters', type=int, default=100)
    p.add_argument('--vlad_init_seed', type=int, default=0)
    # hard negative mining (:1288-1293)
    p.add_argument('--mining_step', type=int, default=250)
    p.add_argument('--mining_cache_size', type=int, default=1000)
    # cadence, validation loss and localisation testing (:1296-1300)
    p.add_argument('--eval_step', type=int, default=100)
    p.add_argument('--save_step', type=int, default=500)
    p.add_argument('--num_eval_queries', type=int, default=50)
    p.add_argument('--eval_ref_r', default=5, type=int)
    # data set names (:1303-1307) and locations (:1226-1231)
    p.add_argument('--local_ref_set', default='train_ref')
    p.add_argument('--local_query_set', default='train_query')
    p.add_argument('--other_ref_set', default='test_ref')
    p.add_argument('--other_query_set', default='test_query')
    p.add_argument('--train_ref_r', default=1, type=int)
    p.add_argument('--img_root', default='')
    p.add_argument('--anchor_root', default='',
                   help='directory of the anchor lists <local_ref_set>_<train_ref_r>_<epoch:03d>.csv '
                        '(column idx; train/train.py:1007-1009); empty: a seeded permutation of '
                        'every train_ref_r-th image')
    p.add_argument('--loc_ref_root', default='',
                   help='directory of the localisation reference lists <ref_set>_<eval_ref_r>.csv '
                        '(train/train.py:1158); empty: every eval_ref_r-th image of the set')
    p.add_argument('--shuffled_root', default='',
                   help='directory of the per-epoch lists <set>_<epoch:03d>.csv; empty: synthetic')
    p.add_argument('--loader_processes', type=int, default=0,
                   help='worker processes decoding the frames of --shuffled_root sets (0: threads only). '
                        'Created before the device is initialised; ignored when it already is')
    p.add_argument('--frame_cache_mb', type=float, default=0.0,
                   help='> 0: keep every frame of the --shuffled_root sets on the device as uint8, up to '
                        'this many MiB, and assemble the batches there (train/frame_bank.py); a frame is '
                        'then decoded, resized and uploaded once per run.  Same batches bit for bit')
    p.add_argument('--force_dist', type=int, default=0,
                   help='single process only: form a ONE-rank RCCL process group and take the data-parallel '
                        'routes through it (the collective path on a one-GPU box)')
    p.add_argument('--dist_timeout', type=float, default=300.0,
                   help='seconds: rendezvous and every collective')
    p.add_argument('--tensorboard', type=int, default=1,
                   help='TensorBoard event files <out>/local and <out>/other with the reference\'s tags '
                        '(train/train.py:304, 380-397, 929-932, 1139-1147)')
    p.add_argument('--save_examples', type=int, default=-1,
                   help='curve PDFs and example pictures of every localisation check (train/train.py:368-420): '
                        '1 / 0; -1 = with --shuffled_root only')
    p.add_argument('--synthetic_dataset', type=int, default=0,
                   help='M > 0: train on a synthetic pose-tagged set of M images through the '
                        'sampler / pipeline / mining / evaluation route')
    p.add_argument('--synthetic_distractor', type=float, default=0.0,
                   help='synthetic set: share of the image contrast that is place-independent')
    # synthetic stand-in for the dataset pipeline
    p.add_argument('--steps', type=int, default=10, help='steps per epoch')
    p.add_argument('--height', type=int, default=180)
    p.add_argument('--width', type=int, default=240)
    p.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    p.add_argument('--seed', type=int, default=42)
    return p


def distance_type(loss):
    """train/train.py:1378-1391."""
    if 'pairwise' in loss:
        return 'pairwise'
    if 'distance' in loss:
        return 'anchor'
    if 'swrd' in loss:
        return 'swrd'
    if 'wrd' in loss:
        return 'wrd'
    if 'wms' in loss:
        return 'wms'
    if 'logratio' in loss:
        return 'logratio'
    return 'none'


def tuple_shape_for(loss, positives, negatives):
    """train/train.py:589-594: quadruplet losses turn the last negative into 'other'."""
    if 'quadruplet' in loss:
        return [1, positives, negatives - 1, 1]
    return [1, positives, negatives]


def get_learning_rate(epoch, flags):
    """train/train.py:118-121."""
    lr = flags.base_lr * (flags.lr_down_factor ** (epoch // flags.lr_down_frequency))
    return max(lr, flags.minimal_lr)


# reduction modes of the reference whose modules are absent from it
UNAVAILABLE_REDUCTIONS = {'spp': 'learnlarge.model.mac', 'pca': 'learnlarge.model.incremental_skl'}

SUPPORTED_LOSSES = ('triplet', 'lazy_triplet', 'evil_triplet', 'quadruplet', 'lazy_quadruplet',
                    'evil_quadruplet', 'ms_loss', 'wms', 'logratio',
                    'distance_triplet', 'distance_lazy_triplet', 'distance_quadruplet',
                    'distance_lazy_quadruplet', 'huber_distance_triplet',
                    'huber_distance_lazy_triplet', 'huber_distance_quadruplet',
                    'huber_distance_lazy_quadruplet', 'wrd', 'prodwrd', 'sumwrd',
                    'residual_trace', 'ntuplet_evmm', 'ntuplet_trace', 'ms_sum')

# losses that take the reference's default ``dimensions = 10`` singular values of EACH side
SIDE_DIMENSIONS_LOSSES = ('residual_trace', 'ms_sum')
SIDE_DIMENSIONS = 10


def guarded_step(opt, guard):
    """The update of one step, after buckets.finish().  With --skip_nonfinite, one pass over the flat
    gradient buffer first (scl_grad_stats): its flag is the optimizer's skip word, so a step with a
    non-finite gradient leaves weights, slots and step count as they were — decided on the device,
    nothing waits here."""
    if guard is not None:
        guard.run()
    opt.step()


def guard_fields(guard, step=None):
    """grad_norm / skipped of the step record (read where the loop waits for the loss anyway); a
    skipped step prints one line."""
    if guard is None:
        return {}
    sumsq, bad = guard.read()
    if bad:
        print('Skipped step{}: {} non-finite gradient values'.format('' if step is None else ' %d' % step, bad))
    return {'grad_norm': float(np.sqrt(sumsq)), 'skipped': int(bad > 0)}


def check_tuple_sizes(flags):
    """Refuse, before the first step, a tuple whose sides have fewer rows than the loss takes
    singular values (the reference's tf.slice fails in the first session run)."""
    if flags.loss in SIDE_DIMENSIONS_LOSSES:
        for name in ('positives_per_tuple', 'negatives_per_tuple'):
            if getattr(flags, name) < SIDE_DIMENSIONS:
                raise SystemExit('--loss %s takes the %d largest singular values of each side: --%s %d is '
                                 'below %d' % (flags.loss, SIDE_DIMENSIONS, name, getattr(flags, name),
                                               SIDE_DIMENSIONS))


def tuple_labels(flags, tuples, first=0):
    """The class labels of ms_loss / ms_sum (train/train.py:822-826, 830-834) for ``tuples``
    tuples, numbered from tuple ``first``: 0 for the anchor and its positives, one class per
    negative, shifted by negatives_per_tuple + 1 per tuple."""
    one = np.concatenate((np.zeros(1 + flags.positives_per_tuple),
                          np.arange(flags.negatives_per_tuple) + 1))
    return np.concatenate([one + (k + first) * (flags.negatives_per_tuple + 1) for k in range(tuples)])


def compute_loss(flags, tuple_shape, output, distances, local_rows=None, group=None):
    """The loss dispatch of build_model (train/train.py:700-855) on ``output`` [T*S, E]."""
    t = flags.tuples_per_batch
    s = sum(tuple_shape)
    loss = flags.loss
    if loss in ('ms_loss', 'wms') and group is not None:
        if loss == 'wms':
            return parallel.wms_loss_dp(distances, output, flags.alpha, flags.beta, group=group,
                                        wfunction=flags.wfunction, sumfunction=flags.sumfunction)
        return parallel.ms_loss_dp(distances, output, group=group, ms_mining=flags.msmining)
    if loss == 'ms_sum' and group is not None:
        # ms_loss on the gathered batch, residual_det on this rank's tuples (mean over ranks)
        ms = parallel.ms_loss_dp(distances, output, group=group, ms_mining=flags.msmining)
        outs = torch.split(output.reshape(t, s, -1), tuple_shape, dim=1)
        det = parallel.tuple_loss_dp(losses.residual_det_loss(outs[0], outs[1], outs[2], flags.margin_1),
                                     group)
        return ms * 5.0 + det
    if group is not None and loss in SUPPORTED_LOSSES:
        # per-tuple losses shard by tuple: the local mean, then the mean over ranks
        return parallel.tuple_loss_dp(compute_loss(flags, tuple_shape, output, distances), group)
    outs = torch.split(output.reshape(t, s, -1), tuple_shape, dim=1)       # :654
    if loss == 'triplet':
        return pointnetvlad_cls.triplet_loss(outs[0], outs[1], outs[2], flags.margin_1)
    if loss == 'lazy_triplet':
        return pointnetvlad_cls.lazy_triplet_loss(outs[0], outs[1], outs[2], flags.margin_1)
    if loss == 'evil_triplet':
        return losses.evil_triplet_loss(outs[0], outs[1], outs[2], flags.margin_1)
    if loss == 'quadruplet':
        return pointnetvlad_cls.quadruplet_loss(outs[0], outs[1], outs[2], outs[3],
                                                flags.margin_1, flags.margin_2)
    if loss == 'lazy_quadruplet':
        return pointnetvlad_cls.lazy_quadruplet_loss(outs[0], outs[1], outs[2], outs[3],
                                                     flags.margin_1, flags.margin_2)
    if loss == 'evil_quadruplet':
        return losses.evil_quadruplet_loss(outs[0], outs[1], outs[2], outs[3], flags.margin_1,
                                           flags.margin_2)
    if loss in SUPPORTED_LOSSES and 'distance' in loss:                        # :719-763
        d_max_squared = float(flags.max_pos_radius) ** 2                       # :695
        f_max_squared = 2.0                                                    # :696
        trip = 'lazy_triplet_loss' if 'lazy' in loss else 'triplet_loss'
        dist = 'huber_distance_loss' if 'huber' in loss else 'distance_loss'
        if 'quadruplet' in loss:
            return losses.distance_quadruplet_loss(outs[0], outs[1], outs[2], outs[3],
                                                   flags.margin_1, flags.margin_2, flags.lam,
                                                   distances, d_max_squared, f_max_squared, trip,
                                                   dist)
        return losses.distance_triplet_loss(outs[0], outs[1], outs[2], flags.margin_1, flags.lam,
                                            distances, d_max_squared, f_max_squared, trip, dist)
    if loss == 'ms_loss':
        return losses.ms_loss(distances, output, ms_mining=flags.msmining)     # :821-827
    if loss == 'wms':
        # only d_alpha, d_beta, wfunction, sumfunction are forwarded (:851-852)
        return losses.wms_loss(distances, output, d_alpha=flags.alpha, d_beta=flags.beta,
                               wfunction=flags.wfunction, sumfunction=flags.sumfunction)
    if loss in ('wrd', 'prodwrd', 'sumwrd'):
        # distances [T, 2(P+N)]: the positive-side weights of all rows, then the negative-side
        # ones (:677-681); only margin_1 is forwarded (:842-849)
        others = flags.positives_per_tuple + flags.negatives_per_tuple
        pos_w, neg_w = torch.split(distances.reshape(t, 2 * others, -1), [others, others], 1)
        fn = {'wrd': losses.wrd_loss, 'prodwrd': losses.prodwrd_loss,
              'sumwrd': losses.sumwrd_loss}[loss]
        return fn(outs[0], outs[1], outs[2], pos_w, neg_w, flags.margin_1)
    if loss in ('ntuplet_evmm', 'ntuplet_trace', 'residual_trace'):            # :780-791
        fn = {'ntuplet_evmm': losses.ntuplet_evmm_loss, 'ntuplet_trace': losses.ntuplet_trace_loss,
              'residual_trace': losses.residual_trace_loss}[loss]
        return fn(outs[0], outs[1], outs[2], flags.margin_1)
    if loss == 'ms_sum':                                                       # :829-837
        return losses.ms_sum(outs[0], outs[1], outs[2], flags.margin_1, distances, output,
                             ms_mining=flags.msmining)
    if loss == 'logratio':
        p = flags.positives_per_tuple
        pos_d, neg_d = torch.split(distances.reshape(t, -1, 1), [p, flags.negatives_per_tuple], 1)
        return losses.logratio_loss(outs[0], outs[1], outs[2], pos_d, neg_d)   # :854-855
    raise ValueError("loss %r is outside the hot path (supported: %s)" % (loss, SUPPORTED_LOSSES))


class SyntheticTuples:
    """Stand-in for get_tuple + load_images (train/train.py:423-582): per step one batch of
    T tuples with the reference's row order and per-loss ``distances`` tensor."""

    def __init__(self, flags, tuple_shape, device, rank=0, world=1):
        self.f, self.shape, self.dev = flags, tuple_shape, device
        self.rank, self.world = rank, world
        self.gen = torch.Generator().manual_seed(flags.seed + rank)
        self.rng = np.random.default_rng(7 + flags.seed)

    def batch(self):
        f = self.f
        t, s = f.tuples_per_batch, sum(self.shape)
        img = torch.randint(0, 256, (t * s, f.height, f.width, 3), generator=self.gen).float()
        dtype = distance_type(f.loss)
        gb = t * s * self.world
        xy = self.rng.uniform(0.0, 200.0, size=(gb, 2))         # same on every rank
        mine = slice(self.rank * t, (self.rank + 1) * t)        # per-tuple payloads: this rank's tuples
        if dtype == 'wms':
            # sklearn pairwise_distances(all, all, 'euclidean') (:557-563), rank-3 [T,S,S]
            d = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(2)).astype(np.float32)[None]
        elif dtype == 'anchor':
            # squared metres anchor -> positives inside max_pos_radius (:529-533), [T,P]
            d = self.rng.uniform(0.0, f.max_pos_radius ** 2,
                                 (t * self.world, f.positives_per_tuple)).astype(np.float32)[mine]
        elif dtype == 'logratio':
            p, n = f.positives_per_tuple, f.negatives_per_tuple      # squared metres (:569-571)
            d = np.concatenate([self.rng.uniform(1, 15 ** 2, (t * self.world, p)),
                                self.rng.uniform(15 ** 2, 200 ** 2, (t * self.world, n))],
                               1).astype(np.float32)[mine]
        elif dtype == 'wrd':
            # weights of the metres anchor -> positives, negatives (:538-556), [T, 2(P+N)]
            p, n = f.positives_per_tuple, f.negatives_per_tuple
            m = np.concatenate([self.rng.uniform(0.5, f.max_pos_radius, (t * self.world, p)),
                                self.rng.uniform(f.min_neg_radius, 200.0, (t * self.world, n))], 1)
            d = np.concatenate([1 / (1 + np.exp(f.alpha * (m - f.beta))),
                                1 / (1 + np.exp(f.alpha * (f.beta - m)))], 1).astype(np.float32)[mine]
        elif f.loss in ('ms_loss', 'ms_sum'):
            # labels built in build_model (:822-826, 830-834), globally unique across ranks
            d = tuple_labels(f, t * self.world)
        else:
            d = None
        dist_t = None if d is None else torch.as_tensor(d).to(self.dev)
        return dist_t, img.to(self.dev)


def batch_distances(flags, distances, device, world=1, rank_offset=0):
    """The sampler's per-anchor payloads -> the tensor ``ops['distances']`` holds for the loss
    (train/train.py:665-691); ms_loss and ms_sum take the labels of :822-826 / :830-834 instead."""
    t = flags.tuples_per_batch
    if flags.loss in ('ms_loss', 'ms_sum'):
        return torch.as_tensor(tuple_labels(flags, t * world, rank_offset)).to(device)
    if distance_type(flags.loss) == 'none':
        return None
    return torch.as_tensor(np.asarray(distances, dtype=np.float32)).to(device)


def cadence_due(step, every, stride, world):
    """Does the cadence `every` (in anchors) fire at anchor position `step`?  One rank: the
    reference's `step % every == 0` (train/train.py:1014, 1070, 1094); several ranks: a step covers
    `stride` = tuples_per_batch * world anchors and the cadence fires when a multiple lies inside it."""
    return step % every == 0 if world == 1 else step % every < stride


def next_cadence(step, every, stride, world, n_anchors):
    """First anchor position after `step` (in steps of `stride`) at which cadence_due fires again,
    capped at `n_anchors`: the end of the window a mining-cache refresh at `step` must cover."""
    nxt = step + stride
    while nxt < n_anchors and not cadence_due(nxt, every, stride, world):
        nxt += stride
    return min(nxt, n_anchors)


def loc_ref_set(flags, ref_set_name):
    """The thinned reference list the localisation check runs against:
    <loc_ref_root>/<ref_set>_<eval_ref_r>.csv (train/train.py:1158)."""
    from . import dataset, frame_bank
    return frame_bank.wrap(
        dataset.CsvImageSet(os.path.join(flags.loc_ref_root,
                                         '{}_{}.csv'.format(ref_set_name, flags.eval_ref_r)),
                            flags.img_root, vlad_cores=flags.vlad_cores, need_yaw=False),
        getattr(flags, 'frame_bank', None))


def open_sets(flags, epoch):
    """(local_ref, local_query, other_ref, other_query) image sets of an epoch."""
    from . import dataset, frame_bank
    if flags.shuffled_root:
        def one(name):
            # (image size: the reference's fixed rule, train/train.py:423-430 — longer side 240 with
            # the NetVLAD head, 180 x 240 cover-and-crop without; --height / --width are the
            # synthetic set's)
            return frame_bank.wrap(
                dataset.CsvImageSet(os.path.join(flags.shuffled_root, '%s_%03d.csv' % (name, epoch)),
                                    flags.img_root, vlad_cores=flags.vlad_cores,
                                    pool=getattr(flags, 'loader_pool', None)),
                getattr(flags, 'frame_bank', None))
        return (one(flags.local_ref_set), one(flags.local_query_set), one(flags.other_ref_set),
                one(flags.other_query_set))
    m = flags.synthetic_dataset
    dis = flags.synthetic_distractor

    def make(num, seed):
        return dataset.SyntheticImageSet(num, flags.height, flags.width, seed=seed, distractor=dis)
    local, other = make(m, flags.seed), make(max(m // 2, 8), flags.seed + 1)
    if dis > 0.0:
        # queries from ANOTHER traverse of the same track (own jitter, noise and distractors), like
        # the reference's query sets: with the references themselves as queries every nearest
        # descriptor is the query's own and the localisation check says 100 % whatever the weights
        return local, make(m, flags.seed + 100), other, make(max(m // 2, 8), flags.seed + 101)
    return local, local, other, other


def train_dataset_epoch(flags, epoch, state, log):
    """``train_one_epoch`` (train/train.py:987-1109) on this process's device.

    With more than one rank (``state['group']``; new work, the reference is single-GPU) a step takes
    ``tuples_per_batch`` anchors PER RANK: rank r trains on anchors [r t, (r + 1) t) of every
    block of world * t, with its own sampler stream (seeded by (epoch, rank), with and without the
    mining cache); a batch dropped on
    one rank ('Faulty training batch') is dropped on all of them (one MIN all-reduce of a flag per
    step), the per-tuple losses become the mean over all ranks' tuples (parallel.tuple_loss_dp),
    the pairwise losses take the gathered batch (for wms the ranks exchange the image indices and
    build the full distance matrix from the poses every rank holds), the mining cache is
    extracted in shards and all-gathered, and rank 0 alone logs and writes checkpoints; the
    evaluations run on every rank alike (no collective inside them)."""
    from . import evaluate, mining
    from .frame_bank import to_device
    from .sampler import InputPipeline, TupleSampler
    model, opt, buckets, saver, dev = (state[k] for k in ('model', 'opt', 'buckets', 'saver', 'dev'))
    guard = state.get('guard')
    group = state.get('group')
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    tuple_shape = state['tuple_shape']
    t, s_img = flags.tuples_per_batch, flags.tuples_per_batch * sum(state['tuple_shape'])
    local_ref, local_query, other_ref, other_query = open_sets(flags, epoch)
    dtype = distance_type(flags.loss)
    dtype = dtype if dtype in ('anchor', 'pairwise', 'wms', 'logratio', 'wrd') else 'none'
    cache = mining.MiningCache()

    def make_sampler(image_set, use_cache):
        return TupleSampler(image_set.xy, image_set.yaw, flags.positives_per_tuple,
                            flags.negatives_per_tuple, flags.max_pos_radius, flags.min_neg_radius,
                            flags.hard_positives_per_tuple, flags.hard_negatives_per_tuple,
                            flags.mutually_exclusive_negs, dtype, cache if use_cache else None,
                            flags.mining_cache_size,
                            np.random.RandomState(42 + epoch if world == 1 else [42 + epoch, rank]),
                            alpha=flags.alpha, beta=flags.beta)
    sampler = make_sampler(local_ref, True)
    other_sampler = make_sampler(other_ref, False)
    pipe = InputPipeline(sampler, local_ref.load_images, tuple_shape, use_hard_negatives=True,
                         depth=2, emit_dropped=True)
    if flags.anchor_root:                                     # train/train.py:1007-1009
        from ..util import io
        anchors = np.array(io.load_csv(os.path.join(
            flags.anchor_root, '{}_{}_{:03d}.csv'.format(flags.local_ref_set, flags.train_ref_r, epoch)))['idx'],
            dtype=int)
        if len(anchors) and (anchors.min() < 0 or anchors.max() >= len(local_ref)):
            raise ValueError('anchor list of epoch %d points outside %s' % (epoch, flags.local_ref_set))
    else:
        anchors = np.random.RandomState(1000 + epoch).permutation(
            np.arange(0, len(local_ref), max(flags.train_ref_r, 1)))
    if flags.steps > 0:
        anchors = anchors[:flags.steps * t * world]           # --steps = batches per rank
    # whole batches only: compute_loss / batch_distances reshape with tuples_per_batch, a short
    # tail batch would raise at the end of the epoch, before the epoch checkpoint is written
    anchors = anchors[:(len(anchors) // (t * world)) * (t * world)]
    lr = get_learning_rate(epoch, flags)
    for g in opt.param_groups:
        g['lr'] = lr
    if rank == 0:
        rec = {'event': 'epoch', 'epoch': epoch, 'anchors': int(len(anchors)),
               'anchor_source': 'list' if flags.anchor_root else 'permutation',
               'first_anchors': [int(a) for a in anchors[:4]], 'learning_rate': lr}
        if state.get('frame_bank') is not None:          # --frame_cache_mb: the bank as the epoch finds it
            rec['frame_bank'] = state['frame_bank'].stats
        log(rec)

    def loss_of(distances, images):
        """Single-process loss (the evaluation on the other region: every rank alike)."""
        out = nets.output(images)
        return compute_loss(flags, tuple_shape, out, batch_distances(flags, distances, dev))

    def train_loss(distances, images, indices):
        out = nets.output(images)
        if group is None:
            return compute_loss(flags, tuple_shape, out, batch_distances(flags, distances, dev))
        if flags.loss == 'wms':
            # the global batch's pairwise geographic distances (train/train.py:557-563) from the
            # poses of ALL ranks' images: the indices travel, every rank holds the poses
            idx_all = parallel.all_gather_ragged(
                torch.as_tensor(np.asarray(indices, dtype=np.int64), device=dev), group).cpu().numpy()
            xy = np.asarray(local_ref.xy, dtype=np.float64)[idx_all]
            dmat = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(2)).astype(np.float32)[None]
            payload = torch.as_tensor(dmat).to(dev)
        elif flags.loss in ('ms_loss', 'ms_sum'):
            payload = batch_distances(flags, distances, dev, world=world)   # globally unique labels
        else:
            payload = batch_distances(flags, distances, dev)
        return compute_loss(flags, tuple_shape, out, payload, group=group)

    def train_on(item):
        have = 0 if item is None else 1
        if group is not None:                                   # a batch dropped anywhere is dropped everywhere
            flag = torch.tensor([have], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            have = int(flag)
        if not have:
            return                                              # 'Faulty training batch'
        distances, images, indices = item
        buckets.zero()
        loss = train_loss(distances, to_device(images, dev), indices)
        loss.backward()
        buckets.finish()
        guarded_step(opt, guard)
        state['step'] += 1
        rec = {'step': state['step'], 'epoch': epoch, 'loss': float(loss.detach()),
               'learning_rate': lr}
        rec.update(guard_fields(guard, state['step']))
        if rank == 0:
            print('Train batch loss: {}'.format(rec['loss']))      # :289
            log(rec)

    def drain(outstanding):
        while outstanding:
            train_on(pipe.get())
            outstanding -= 1
        return 0

    outstanding, mining_count = 0, 0
    try:
        stride = t * world

        def due(every):
            return cadence_due(step, every, stride, world)
        for step in range(0, len(anchors), stride):
            if due(flags.mining_step):                               # :1014-1068
                outstanding = drain(outstanding)
                mining_indices = np.arange(mining_count * flags.mining_cache_size,
                                           (mining_count + 1) * flags.mining_cache_size) % len(local_ref)
                # every anchor trained before the NEXT refresh: with several ranks the cadence fires
                # up to stride - 1 anchors late, so the window runs to the next firing, not to
                # step + mining_step (anchors outside the cache get no hard positives / negatives)
                window_end = next_cadence(step, flags.mining_step, stride, world, len(anchors))
                to_mine = anchors[step:window_end]
                mining_indices = np.concatenate([mining_indices, to_mine])
                if group is None:
                    feats = evaluate.extract_features(model, local_ref, mining_indices, s_img)
                else:                        # each rank embeds a contiguous share, rank order = list order
                    share = np.array_split(mining_indices, world)[rank]
                    feats = parallel.all_gather_ragged(
                        evaluate.extract_features(model, local_ref, share, s_img)
                        if len(share) else torch.zeros((0, 0), device=dev), group)   # (width: from the others)
                cache.update(feats, mining_indices)
                mining_count += 1
                if rank == 0:
                    log({'step': state['step'], 'event': 'mining_cache', 'images': int(len(mining_indices)),
                         'anchor_window': [int(step), int(window_end)]})
            if due(flags.eval_step):                                 # :1070-1092
                outstanding = drain(outstanding)
                if rank == 0:
                    saver.save_rolling(model, state['step'], opt)
                test_number = state['step'] // flags.eval_step
                nq = (flags.num_eval_queries // t) * t
                test_idx = np.arange(test_number * nq, (test_number + 1) * nq) % len(other_ref)
                with torch.no_grad():
                    ev, used = evaluate.eval_loss(loss_of, other_sampler, other_ref, test_idx, t,
                                                  tuple_shape, dev)
                rec = {'step': state['step'], 'event': 'eval', 'other_region_loss': ev,
                       'eval_batches': used}
                for mode, rset, qset, rname in (('other', other_ref, other_query, flags.other_ref_set),
                                                ('local', local_ref, local_query, flags.local_ref_set)):
                    if flags.loc_ref_root and flags.shuffled_root:     # train/train.py:1158-1167
                        rset = loc_ref_set(flags, rname)
                        refs = np.arange(len(rset))
                    else:
                        refs = np.arange(0, len(rset), max(flags.eval_ref_r, 1))
                    q = np.arange(test_number * flags.num_eval_queries,
                                  (test_number + 1) * flags.num_eval_queries) % len(qset)
                    want = (flags.save_examples if flags.save_examples >= 0 else bool(flags.shuffled_root)) \
                        and rank == 0
                    out_name = '{:02d}_checkpoint-{}'.format(epoch, state['step'])   # :1079-1080
                    metrics, nearest = evaluate.evaluate_localization(
                        model, rset, refs, qset, q, s_img,
                        plots=(saver.out_dir, mode, out_name) if want else None)    # :368-396
                    rec[mode] = metrics
                    if want:                                         # :400-420
                        evaluate.save_example_pictures(saver.out_dir, mode, out_name, qset, q, rset, refs,
                                                       nearest)
                if rank == 0:
                    print('Other region loss: {}'.format(ev))        # :1144
                    log(rec)
            if due(flags.save_step):                                 # :1094-1102
                outstanding = drain(outstanding)
                if rank == 0:
                    saver.save_part(model, state['step'], opt)
            pipe.put(anchors[step + rank * t:step + (rank + 1) * t])
            outstanding += 1
            if outstanding > 1:                                      # one batch stays in flight
                train_on(pipe.get())
                outstanding -= 1
        drain(outstanding)
    except Exception:
        # a failure on ONE rank (a worker error re-raised by pipe.get(), a bad batch) would leave
        # the others blocked in the per-step MIN all-reduce: take the process group down with it
        # (no destroy_process_group() first: with RCCL it can block behind this rank's outstanding
        # collectives while the peers wait in theirs — a hang is not an exception)
        if group is not None and os.environ.get('SCL_TRAIN_ABORT_ON_RANK_FAILURE', '1') != '0':
            try:
                pipe.close()
                if getattr(flags, 'loader_pool', None) is not None:
                    flags.loader_pool.shutdown()
                for b in (state.get('boards') or {}).values():
                    b.close()
            except Exception:
                pass
            parallel.abort_rank(1)        # peers see the closed connection instead of waiting
        raise
    finally:
        pipe.close()
    if rank == 0:
        saver.save_epoch(model, epoch, state['step'], opt)           # :984


def restore(flags, model, opt, verbose=True):
    """--checkpoint: restore_weights (train/train.py:882-905) takes the variables of the
    ``vgg16_netvlad_pca`` scope only, so a dense reduction head starts from its initialiser (logged
    as 'Newly initialized: <var>', :889); --resume also restores the head and every Adam slot and
    returns the global step.  Returns the step to continue from."""
    if not flags.checkpoint:
        return 0
    if getattr(flags, 'vlad_init', 'none') == 'kmeans':
        # the head is about to be seeded from data: a checkpoint without the two head variables
        # (and with nothing else missing) will do; flags.vlad_init_found says whether it had them
        from ..model import vlad_init
        _, missing = vlad_init.load_without_head(model, flags.checkpoint, head=False)
        flags.vlad_init_found = not missing
        if reduction.head_of(model) is not None and verbose:
            for name, _ in reduction.head_of(model).tf_variables():
                print('Newly initialized: {}'.format(name))
        return 0
    got = checkpoint.load(model, flags.checkpoint, optimizer=opt if flags.resume else None,
                          head=flags.resume)
    head = reduction.head_of(model)
    if not flags.resume and head is not None and verbose:
        for name, _ in head.tf_variables():
            print('Newly initialized: {}'.format(name))
    return got if flags.resume else 0


def check_vlad_init(flags):
    """--vlad_init kmeans needs a head to seed, frames to seed it from, and a run that starts."""
    if flags.vlad_init != 'kmeans':
        return
    if flags.vlad_cores != 64:
        raise SystemExit('--vlad_init kmeans seeds the NetVLAD head: it needs --vlad_cores 64')
    if not (flags.synthetic_dataset > 0 or flags.shuffled_root):
        raise SystemExit('--vlad_init kmeans takes its frames from the training set: it needs '
                         '--synthetic_dataset M or --shuffled_root DIR')
    if flags.resume:
        raise SystemExit('--vlad_init kmeans would replace the head --resume restores (and keep its '
                         'optimizer slots): seed the head in a run that starts, or drop one of the two')
    if flags.vlad_init_images < 1 or flags.vlad_init_per_image < 1 or flags.vlad_init_iters < 1:
        raise SystemExit('--vlad_init_images, --vlad_init_per_image and --vlad_init_iters must be positive')


def seed_vlad_head(flags, model, tuple_shape):
    """--vlad_init kmeans, after the restore and before the first step: ``vlad_init.init_head`` on the
    first --vlad_init_images entries of a seeded permutation of epoch 0's local reference set.
    Every rank runs it alike: the frames, the seeds and the restored weights are the same on all of
    them and the kernels fix every summation order, so the ranks hold the same head bit for bit
    without a collective.  Returns the log record."""
    from ..model import vlad_init
    local_ref = open_sets(flags, 0)[0]
    indices = np.random.RandomState(flags.vlad_init_seed).permutation(len(local_ref))[:flags.vlad_init_images]
    rec = vlad_init.init_head(model, local_ref, indices, flags.tuples_per_batch * sum(tuple_shape),
                              per_image=flags.vlad_init_per_image, iters=flags.vlad_init_iters,
                              seed=flags.vlad_init_seed)
    out = {'event': 'vlad_init', 'images': int(len(indices))}
    out.update(rec)
    out['replaced_checkpoint_head'] = bool(getattr(flags, 'vlad_init_found', False))
    return out


def main(argv=None):
    flags = make_parser().parse_args(argv)
    if flags.reduction in UNAVAILABLE_REDUCTIONS:
        raise SystemExit('--reduction %s needs %s, which the reference does not contain'
                         % (flags.reduction, UNAVAILABLE_REDUCTIONS[flags.reduction]))
    if flags.vlad_cores not in (0, 64) or flags.reduction not in ('none',) + reduction.KINDS:
        raise SystemExit('only --vlad_cores 64 | 0 with --reduction none|1fc|2fc|3fc is on the hot path')
    check_tuple_sizes(flags)
    check_vlad_init(flags)
    if flags.skip_nonfinite and flags.optimizer_impl != 'hip':
        raise SystemExit('--skip_nonfinite 1 needs --optimizer_impl hip: the skip is decided on the device, '
                         'inside the update kernel')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    # TEST ONLY (SCL_TRAIN_ONE_GPU_GLOO=1): every rank on cuda:0 with gloo carrying the collectives —
    # the data-parallel routes on a one-GPU box (tests/test_gpu_dist.py)
    one_gpu = os.environ.get('SCL_TRAIN_ONE_GPU_GLOO') == '1'
    if one_gpu:
        local_rank = 0
    # worker processes for the image files: spawned BEFORE anything touches the device
    flags.loader_pool = None
    if flags.shuffled_root and flags.loader_processes > 0:
        from . import dataset
        flags.loader_pool = dataset.make_loader_pool(flags.loader_processes)
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if flags.force_dist and world != 1:
        raise SystemExit('--force_dist is the one-rank form of the collective path')
    group = parallel.init_process_group(dev, backend='gloo' if one_gpu else 'nccl',
                                        timeout_s=flags.dist_timeout, force_single=bool(flags.force_dist))

    np.random.seed(42)                                    # train/train.py:1463-1464
    tuple_shape = tuple_shape_for(flags.loss, flags.positives_per_tuple,
                                  flags.negatives_per_tuple)
    cdt = torch.bfloat16 if flags.dtype == 'bf16' else torch.float32
    model = nets.set_default_model(nets.VGG16NetVLAD(compute_dtype=cdt,
                                                     vlad_cores=flags.vlad_cores).to(dev))
    if flags.reduction in reduction.KINDS:             # :631-644, float32 under --dtype bf16 too
        reduction.attach(model, flags.reduction, flags.out_dim, height=flags.height, width=flags.width)
    params = nets.trainable_parameters(model)       # train/train.py:606-611: the head decides
    buckets = parallel.GradBuckets(params, group, force_collectives=bool(flags.force_dist))
    nets.GRAD_SINK = buckets       # conv weight / bias gradients go straight into the flat buffer
    # train/train.py:865-870: MomentumOptimizer / AdamOptimizer — TF's Adam (epsilon outside the bias
    # correction), not torch's: train/optim.py
    opt = make_optimizer(flags.optimizer, params, flags.base_lr, flags.momentum, impl=flags.optimizer_impl)
    guard = None
    if flags.skip_nonfinite:             # one pass over the flat gradients; its flag is the skip word
        guard = GradStats(buckets.flat)
        opt.skip_flag = guard.flag
    # restore_weights (:882-905) + the slot variables a tf.train.Saver checkpoint carries
    step = restore(flags, model, opt, verbose=rank == 0)
    out_dir = os.path.join(flags.out_root, flags.out_folder or flags.loss)
    saver = checkpoint.Saver(out_dir, flags.max_to_keep)
    data = SyntheticTuples(flags, tuple_shape, dev, rank, world)
    log = open(os.path.join(out_dir, 'train_log.txt'), 'a') if rank == 0 and (
        os.makedirs(out_dir, exist_ok=True) or True) else None

    # writers['local'] / writers['other'] (train/train.py:929-932): the training loss and learning
    # rate of every step and the training region's localisation numbers / the other region's loss and
    # localisation numbers, as TensorBoard event files (tf_events.py)
    boards = None
    if rank == 0 and flags.tensorboard:
        from .. import tf_events
        boards = {m: tf_events.SummaryWriter(os.path.join(out_dir, m)) for m in ('local', 'other')}

    def to_boards(rec):
        if boards is None:
            return
        if 'loss' in rec and 'event' not in rec:                                  # :304
            boards['local'].add_scalars({'loss': rec['loss'], 'learning_rate': rec['learning_rate']},
                                        rec['step'])
        elif rec.get('event') == 'eval':
            if rec.get('other_region_loss') is not None:                           # :1145-1147
                boards['other'].add_scalars({'loss': rec['other_region_loss']}, rec['step'])
            for mode in ('other', 'local'):                                        # :380-397
                vals = {k: v for k, v in (rec.get(mode) or {}).items() if isinstance(v, (int, float))}
                if vals:
                    boards[mode].add_scalars(vals, rec['step'])
            for b in boards.values():
                b.flush()

    if flags.synthetic_dataset > 0 or flags.shuffled_root:
        # one bank per process for the whole run: the per-epoch lists re-order the same files
        flags.frame_bank = None
        if flags.frame_cache_mb > 0 and flags.shuffled_root:
            from .frame_bank import FrameBank
            flags.frame_bank = FrameBank(int(flags.frame_cache_mb * 2 ** 20), dev)
        state = dict(model=model, opt=opt, buckets=buckets, saver=saver, dev=dev,
                     tuple_shape=tuple_shape, step=step, group=group, boards=boards,
                     frame_bank=flags.frame_bank, guard=guard)

        def write(rec):
            if log is not None:
                log.write(json.dumps(rec) + '\n')
                log.flush()
            to_boards(rec)
        try:
            if flags.vlad_init == 'kmeans':
                write(seed_vlad_head(flags, model, tuple_shape))
            for epoch in range(flags.max_epoch):
                train_dataset_epoch(flags, epoch, state, write)
        finally:
            nets.GRAD_SINK = None        # also after an exception: the sink outlives nothing
            for b in (boards or {}).values():
                b.close()
            if flags.loader_pool is not None:
                flags.loader_pool.shutdown()
            if flags.frame_bank is not None:
                state['frame_bank_stats'] = flags.frame_bank.stats
                flags.frame_bank.close()
        return state

    for epoch in range(flags.max_epoch):
        lr = get_learning_rate(epoch, flags)
        for g in opt.param_groups:
            g['lr'] = lr
        for _ in range(flags.steps):
            t0 = time.time()
            distances, img = data.batch()
            buckets.zero()
            output = nets.output(img)                             # ops['output'] (:606-644)
            loss = compute_loss(flags, tuple_shape, output, distances, group=group)
            loss.backward()
            buckets.finish()
            guarded_step(opt, guard)
            step += 1
            if rank == 0:
                rec = {'step': step, 'epoch': epoch, 'loss': float(loss.detach()),
                       'learning_rate': lr, 'sec': round(time.time() - t0, 4)}
                rec.update(guard_fields(guard, step))
                print('Train batch loss: {}'.format(rec['loss']))   # :289
                log.write(json.dumps(rec) + '\n')
                log.flush()
                to_boards(rec)
                if step % flags.eval_step == 0:
                    saver.save_rolling(model, step, opt)              # :1079
                if step % flags.save_step == 0:
                    saver.save_part(model, step, opt)                 # :1102
        if rank == 0:
            saver.save_epoch(model, epoch, step, opt)                 # :984
    nets.GRAD_SINK = None
    for b in (boards or {}).values():
        b.close()
    if group is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

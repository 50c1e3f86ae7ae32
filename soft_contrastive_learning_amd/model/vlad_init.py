"""A NetVLAD head from data: k-means on conv5_3 descriptors, then the head every NetVLAD
implementation builds from the clusters.

The reference always warm-starts from a released model that contains a head, so it has no such
step; a backbone trained without one (``--vlad_cores 0``), or a head for a new domain, needs it:

* cluster a sample of the L2-normalised conv5_3 descriptors (``kmeans``; csrc/kmeans.hip),
* ``cluster_centers = -c`` — this package's head adds its centres (``x + C``, oracle/netvlad_np.py),
  so the residual to the centre c is obtained with C = -c,
* ``assignment_kernel = alpha c / |c|`` with the softmax sharpness alpha chosen from the data: at
  the MEAN gap between a descriptor's best and second-best normalised centre the second soft
  assignment is 0.01 of the first, ``alpha = -ln(0.01) / mean(best - second)``.

**Definition of a Lloyd step** (``assign_np`` / ``kmeans_step_np`` are its executable statement in
float64; include/scl_hip.h says how the kernels round).  With offsets ``off_k``:
``score[n, k] = x_n . c_k - off_k``.  A score takes part unless it is a NaN or ``-inf`` (``+inf``
does).  ``label[n]`` is the k of the largest score that takes part, the lowest k on a tie, ``-1``
where none does; ``best[n]`` is that score and ``second[n]`` the next one in the order (score
descending, k ascending), each ``-inf`` where there is none (``second`` always at K = 1).  With
``off_k = |c_k|^2 / 2`` the largest score is the nearest centre: ``|x - c|^2 = |x|^2 - 2 score``.
The new centre of cluster k is the mean of its rows; a cluster without rows keeps its centre.  The
inertia of the step is ``sum |x_n|^2 - 2 best[n]`` over the labelled rows: the squared distances
to the centres the step STARTED from.

Limits: float32 only, D = 512, K <= 64, seeding with random rows (no k-means++), an empty cluster
keeps its centre (no splitting).  HIP device only; there is no CPU fallback.

Script::

    python -m soft_contrastive_learning_amd.model.vlad_init --checkpoint IN --out OUT \\
        (--csv_root DIR --set train_ref --img_root DIR | --synthetic N --height H --width W) \\
        [--images 500 --per_image 100 --iters 100 --seed 0]

reads IN (a head in it is optional), seeds the head and writes the checkpoint stem OUT, which
``evaluation.inference`` and ``train.train --checkpoint`` load strictly.
"""
import argparse
import collections
import math
import os

import numpy as np
import torch

from .. import _lib as L

D = L.VLAD_D
HEAD_NAMES = ('assignment/kernel', 'cluster_centers')
CHECK_EVERY = 10           # iterations between two looks at the early-stop counters (a host sync each)

KMeansResult = collections.namedtuple('KMeansResult', 'centres labels counts inertia empty iterations')


# ---- the host statement ----------------------------------------------------------------------------

def assign_np(x, centres, offsets):
    """(label int32 [N], best float64 [N], second float64 [N]) of the definition above."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64)
    off = np.asarray(offsets, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        score = x @ c.T - off[None, :]
    takes_part = ~np.isnan(score) & (score > -np.inf)
    v = np.where(takes_part, score, -np.inf)
    rows = np.arange(len(x))
    label = np.argmax(v, axis=1)                     # the first of equal values: the lowest k
    best = v[rows, label]
    v[rows, label] = -np.inf
    second = v.max(axis=1)
    label = np.where(takes_part.any(axis=1), label, -1).astype(np.int32)
    return label, best, second


def offsets_np(centres):
    """``|c_k|^2 / 2`` in float64, rounded once to float32."""
    c = np.asarray(centres, dtype=np.float64)
    return (0.5 * (c * c).sum(axis=1)).astype(np.float32)


def kmeans_step_np(x, centres, labels=None):
    """One Lloyd step from ``centres`` -> (new centres float32 [K, 512], labels int32 [N], counts
    int32 [K], inertia float64).  ``labels``: take these instead of the step's own assignment (the
    update and the inertia of somebody else's labels, for the tests: ``best`` is then the score at
    the given label)."""
    x64 = np.asarray(x, dtype=np.float64)
    old = np.asarray(centres, dtype=np.float32)
    off = offsets_np(old)
    if labels is None:
        labels, best, _ = assign_np(x64, old, off)
    else:
        labels = np.asarray(labels, dtype=np.int32)
        at = np.maximum(labels, 0)
        best = (x64 * old.astype(np.float64)[at]).sum(axis=1) - off.astype(np.float64)[at]
    k = len(old)
    on = labels >= 0
    counts = np.bincount(labels[on], minlength=k).astype(np.int32)
    sums = np.zeros((k, x64.shape[1]), dtype=np.float64)
    np.add.at(sums, labels[on], x64[on])
    new = old.copy()
    filled = counts > 0
    new[filled] = (sums[filled] / counts[filled, None]).astype(np.float32)
    inertia = float(((x64[on] * x64[on]).sum(axis=1) - 2.0 * best[on]).sum())
    return new, labels, counts, inertia


def _alpha_of(best, second, labels):
    """-ln(0.01) / mean gap, the mean in float64 on the host over the labelled rows."""
    on = np.asarray(labels) >= 0
    if not on.any():
        raise ValueError('head_from_centres: no descriptor has a nearest centre')
    gap = float((np.asarray(best, dtype=np.float64)[on] - np.asarray(second, dtype=np.float64)[on]).mean())
    if not (gap > 0.0) or not math.isfinite(gap):
        raise ValueError('head_from_centres: the mean gap between the two nearest centres is %r, '
                         'not positive' % gap)
    return -math.log(0.01) / gap, gap


def _unit_np(centres):
    c = np.asarray(centres, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != D or c.shape[0] < 2:
        raise ValueError('head_from_centres needs centres [K, %d] with K >= 2, got %s' % (D, c.shape))
    norm = np.sqrt((c * c).sum(axis=1))
    if not (norm > 0.0).all():
        raise ValueError('head_from_centres: a centre has zero norm')
    return (c / norm[:, None]).astype(np.float32)


def head_from_centres_np(centres, x):
    """The host statement of ``head_from_centres``: NumPy in, NumPy out."""
    c = np.asarray(centres, dtype=np.float32)
    unit = _unit_np(c)
    label, best, second = assign_np(x, unit, np.zeros(len(unit), dtype=np.float32))
    alpha, _ = _alpha_of(best, second, label)
    k = len(c)
    return ((np.float32(alpha) * unit).T.reshape(1, 1, D, k).copy(),
            (-c).T.reshape(1, 1, 1, D, k).copy(), alpha)


# ---- the device ------------------------------------------------------------------------------------

def partials(n):
    """G of an N-row call: workgroups, and rows of the partial arrays (a function of N alone)."""
    return -(-int(n) // L.KMEANS_ROWS)


def _rows(x, name='x'):
    L.require_device(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1:
        raise ValueError('%s must be float32 [., %d] with at least one row, got %s %s'
                         % (name, D, x.dtype, tuple(x.shape)))
    return x.contiguous()


class _Scratch:
    """Everything a run of Lloyd steps on one (N, K, device) writes, allocated once."""

    def __init__(self, n, k, dev, sums):
        g = partials(n)
        self.n, self.k, self.g = n, k, g
        self.best = torch.empty(n, dtype=torch.float32, device=dev)
        self.second = torch.empty(n, dtype=torch.float32, device=dev)
        nbytes = L.load().scl_kmeans_workspace_bytes(n, k)
        if nbytes == 0:
            raise ValueError('k-means has no kernel for N=%d, K=%d (N <= %d, 1 <= K <= %d)'
                             % (n, k, L.KMEANS_MAX_N, L.VLAD_K))
        self.work = L.workspace(nbytes, dev)
        if sums:
            self.part_sum = torch.empty((g, k, D), dtype=torch.float32, device=dev)
            self.part_cnt = torch.empty((g, k), dtype=torch.int32, device=dev)
            self.part_inertia = torch.empty(g, dtype=torch.float64, device=dev)
            self.counts = torch.empty(k, dtype=torch.int32, device=dev)
        else:
            self.part_sum = self.part_cnt = self.part_inertia = self.counts = None


def _assign(x, centres, offsets, label, s):
    with torch.cuda.device(x.device):
        L.check(L.load().scl_kmeans_assign(
            L.ptr(x), s.n, L.ptr(centres), L.ptr(offsets), s.k, L.ptr(label), L.ptr(s.best), L.ptr(s.second),
            L.ptr(s.part_sum), L.ptr(s.part_cnt), L.ptr(s.part_inertia), L.ptr(s.work), s.work.numel(),
            L.stream_of(x)))


def _update(s, old, new, inertia):
    with torch.cuda.device(old.device):
        L.check(L.load().scl_kmeans_update(
            L.ptr(s.part_sum), L.ptr(s.part_cnt), L.ptr(s.part_inertia), s.g, s.k, L.ptr(old), L.ptr(new),
            L.ptr(s.counts), L.ptr(inertia), L.stream_of(old)))


def assign(x, centres, offsets, sums=False):
    """One ``scl_kmeans_assign`` call on the current stream -> dict of device tensors: ``label``,
    ``best``, ``second`` and, with ``sums``, the per-workgroup partials ``part_sum`` [G, K, 512],
    ``part_cnt`` [G, K], ``part_inertia`` [G]."""
    x = _rows(x)
    centres = _rows(centres, 'centres')
    L.require_device(offsets)
    k = centres.shape[0]
    if offsets.dtype != torch.float32 or tuple(offsets.shape) != (k,):
        raise ValueError('offsets must be float32 [%d], got %s %s' % (k, offsets.dtype, tuple(offsets.shape)))
    s = _Scratch(x.shape[0], k, x.device, sums)
    label = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    _assign(x, centres, offsets.contiguous(), label, s)
    out = {'label': label, 'best': s.best, 'second': s.second}
    if sums:
        out.update(part_sum=s.part_sum, part_cnt=s.part_cnt, part_inertia=s.part_inertia)
    return out


def update(part_sum, part_cnt, part_inertia, old_centres):
    """One ``scl_kmeans_update`` call -> (new centres float32 [K, 512], counts int32 [K], inertia
    float64 [1]) device tensors."""
    L.require_device(part_sum, part_cnt, part_inertia, old_centres)
    old = _rows(old_centres, 'old_centres')
    g, k = part_cnt.shape
    if (tuple(part_sum.shape) != (g, k, D) or tuple(part_inertia.shape) != (g,) or old.shape[0] != k
            or part_sum.dtype != torch.float32 or part_cnt.dtype != torch.int32
            or part_inertia.dtype != torch.float64):
        raise ValueError('update: partials [G, K, %d] float32 / [G, K] int32 / [G] float64 and centres '
                         '[K, %d] do not fit' % (D, D))
    s = _Scratch.__new__(_Scratch)
    s.g, s.k = g, k
    s.part_sum, s.part_cnt, s.part_inertia = part_sum.contiguous(), part_cnt.contiguous(), part_inertia.contiguous()
    s.counts = torch.empty(k, dtype=torch.int32, device=old.device)
    new = torch.empty_like(old)
    inertia = torch.empty(1, dtype=torch.float64, device=old.device)
    _update(s, old, new, inertia)
    return new, s.counts, inertia


def device_offsets(centres):
    """``|c_k|^2 / 2``: the sum in float64, rounded once to float32."""
    c = centres.double()
    return (0.5 * (c * c).sum(dim=1)).float()


def kmeans(x, k, iters=100, seed=0, tol=0.0, seed_rows=None):
    """Lloyd's algorithm on the rows of ``x`` (float32 [N, 512] on a HIP device, N >= k) ->
    ``KMeansResult(centres [k, 512], labels int32 [N], counts int32 [k], inertia float64 [iterations],
    empty, iterations)``; the tensors are on ``x``'s device, ``inertia`` is a NumPy array.

    Seeding: the rows ``np.random.RandomState(seed).permutation(N)[:k]`` (``seed_rows``: these rows
    instead, duplicates allowed — a duplicate loses every tie to its lower twin).  An iteration is one
    assign call with ``off = |c|^2 / 2`` and one update call; ``inertia[i]`` is measured against the
    centres iteration i started from.  The loop stops after ``iters`` iterations, or at the first
    iteration that changed no label — from there on every iteration would reproduce the same bits,
    so the result does not depend on WHEN the stop is noticed: the whole loop is enqueued without
    a host synchronisation, except that every ``CHECK_EVERY`` iterations the host reads the counters
    of changed labels.  ``tol`` > 0 also stops at such a look when the last iteration lowered the
    inertia by no more than ``tol`` times its value.  ``labels`` are the last iteration's: the
    nearest centre among those it started from."""
    x = _rows(x)
    n, k, iters = x.shape[0], int(k), int(iters)
    if not 1 <= k <= L.VLAD_K or n < k or iters < 1:
        raise ValueError('kmeans needs 1 <= k <= %d, N >= k and iters >= 1; got k=%d N=%d iters=%d'
                         % (L.VLAD_K, k, n, iters))
    dev = x.device
    if seed_rows is None:
        seed_rows = np.random.RandomState(seed).permutation(n)[:k]
    seed_rows = np.asarray(seed_rows, dtype=np.int64)
    if seed_rows.shape != (k,) or seed_rows.min() < 0 or seed_rows.max() >= n:
        raise ValueError('seed_rows must be %d rows of x' % k)
    s = _Scratch(n, k, dev, True)
    centres = [x[torch.from_numpy(seed_rows).to(dev)].contiguous(), torch.empty((k, D), dtype=torch.float32, device=dev)]
    labels = [torch.full((n,), -2, dtype=torch.int32, device=dev) for _ in range(2)]
    inertia = torch.zeros(iters, dtype=torch.float64, device=dev)
    changed = torch.zeros(iters, dtype=torch.int64, device=dev)
    done = iters
    for it in range(iters):
        cur, nxt = it & 1, (it + 1) & 1
        _assign(x, centres[cur], device_offsets(centres[cur]), labels[cur], s)
        _update(s, centres[cur], centres[nxt], inertia[it:it + 1])
        changed[it] = (labels[cur] != labels[nxt]).sum()
        if (it + 1) % CHECK_EVERY == 0 and it + 1 < iters:
            ch = changed[:it + 1].cpu().numpy()
            still = np.flatnonzero(ch == 0)
            if len(still):
                done = int(still[0]) + 1
                break
            if tol > 0.0:
                last = inertia[it - 1:it + 1].cpu().numpy()
                if last[0] - last[1] <= tol * abs(last[1]):
                    done = it + 1
                    break
    ran = it + 1
    ch = changed[:ran].cpu().numpy()
    still = np.flatnonzero(ch == 0)
    if len(still):
        done = min(done, int(still[0]) + 1)
    done = min(done, ran)
    counts = s.counts.clone()
    return KMeansResult(centres[ran & 1], labels[(ran - 1) & 1], counts, inertia[:done].cpu().numpy(),
                        int((counts == 0).sum()), done)


def head_from_centres(centres, x):
    """centres [K, 512], x [N, 512] (float32 device tensors) -> (assignment_kernel [1, 1, 512, K],
    cluster_centers [1, 1, 1, 512, K], alpha): one assign call with the normalised centres and zero
    offsets gives every row's best and second-best cosine; the mean of their gap is taken in float64
    on the host.  ``ValueError`` for K < 2, a centre of zero norm, or a mean gap that is not
    positive."""
    x = _rows(x)
    centres = _rows(centres, 'centres')
    k = centres.shape[0]
    if k < 2:
        raise ValueError('head_from_centres needs K >= 2, got %d' % k)
    c64 = centres.double()
    norm = (c64 * c64).sum(dim=1).sqrt()
    if not bool((norm > 0).all()):
        raise ValueError('head_from_centres: a centre has zero norm')
    unit = (c64 / norm[:, None]).float().contiguous()
    got = assign(x, unit, torch.zeros(k, dtype=torch.float32, device=x.device))
    alpha, _ = _alpha_of(got['best'].cpu().numpy(), got['second'].cpu().numpy(), got['label'].cpu().numpy())
    kernel = (unit * float(np.float32(alpha))).t().reshape(1, 1, D, k).contiguous()
    return kernel, (-centres).t().reshape(1, 1, 1, D, k).contiguous(), alpha


def sample_descriptors(model, image_set, indices, images_per_pass, per_image=100, seed=0):
    """``per_image`` positions of the L2-normalised conv5_3 map (``model.forward_vgg16``) of every
    listed frame, drawn without replacement from ``RandomState(seed)`` frame after frame (a smaller
    map gives all of its positions) -> float32 [N, 512] on the model's device."""
    from ..train.frame_bank import to_device
    dev = next(model.parameters()).device
    idx = np.asarray(indices, dtype=int)
    rng = np.random.RandomState(seed)
    rows = []
    with torch.no_grad():
        for s in range(0, len(idx), images_per_pass):
            img = to_device(image_set.load_images(idx[s:s + images_per_pass]), dev)
            fmap = model.forward_vgg16(img).float()
            b, p = fmap.shape[0], fmap.shape[1] * fmap.shape[2]
            fmap = fmap.reshape(b, p, D)
            for i in range(b):
                pos = np.sort(rng.permutation(p)[:per_image])
                rows.append(fmap[i, torch.from_numpy(pos).to(dev)])
    return torch.cat(rows, 0).contiguous()


def init_head(model, image_set, indices, images_per_pass, per_image=100, iters=100, seed=0, details=None):
    """Seed ``model``'s NetVLAD head from the frames ``indices`` of ``image_set``: sample
    descriptors, ``kmeans`` with K = 64, ``head_from_centres``, copy into ``assignment_kernel`` and
    ``cluster_centers`` (nothing else changes).  Runs under ``no_grad``.  Everything is a function of
    the arguments and the weights, so every rank of a data-parallel run that calls it with the same
    arguments gets the same head.  Returns a record: ``N``, ``iterations``, ``inertia_first``,
    ``inertia_last``, ``empty_clusters``, ``alpha``.  ``details``: a dict that receives the sampled
    rows (``x``) and the ``KMeansResult`` (``kmeans``)."""
    if getattr(model, 'vlad_cores', 64) != 64:
        raise ValueError('init_head needs a model with the NetVLAD head (vlad_cores 64)')
    k = L.VLAD_K
    with torch.no_grad():
        x = sample_descriptors(model, image_set, indices, images_per_pass, per_image, seed)
        if x.shape[0] < k:
            raise ValueError('init_head: %d descriptors for %d clusters; list more frames' % (x.shape[0], k))
        res = kmeans(x, k, iters=iters, seed=seed)
        kernel, centers, alpha = head_from_centres(res.centres, x)
        model.assignment_kernel.copy_(kernel)
        model.cluster_centers.copy_(centers)
    if details is not None:
        details.update(x=x, kmeans=res)
    return {'N': int(x.shape[0]), 'iterations': int(res.iterations),
            'inertia_first': float(res.inertia[0]), 'inertia_last': float(res.inertia[-1]),
            'empty_clusters': int(res.empty), 'alpha': float(alpha)}


def load_without_head(model, path, optimizer=None, head=True):
    """``checkpoint.load`` that tolerates a checkpoint without the two head variables — and nothing
    else missing (``KeyError`` as the strict load raises it).  Returns (global step, the names that
    were missing)."""
    from .. import checkpoint
    from .nets import SCOPE
    sd = checkpoint.read_variables(path)
    step = int(np.asarray(sd.get(checkpoint.GLOBAL_STEP_VAR, 0)))
    missing = model.load_state_dict_tf({key: torch.from_numpy(np.ascontiguousarray(v))
                                        for key, v in sd.items() if v.dtype.kind == 'f'},
                                       strict=False, head=head)
    other = [m for m in missing if m not in tuple(SCOPE + '/' + h for h in HEAD_NAMES)]
    if other:
        raise KeyError("checkpoint lacks %s" % other)
    if optimizer is not None:
        checkpoint.restore_optimizer(model, optimizer, sd)
    return step, missing


def make_parser():
    p = argparse.ArgumentParser(description='Seed a NetVLAD head with k-means on conv5_3 descriptors.')
    p.add_argument('--checkpoint', required=True, help='checkpoint to read (its head, if any, is replaced)')
    p.add_argument('--out', required=True, help='checkpoint stem to write')
    p.add_argument('--csv_root', default='', help='directory of <set>.csv')
    p.add_argument('--set', default='train_ref')
    p.add_argument('--img_root', default='')
    p.add_argument('--synthetic', type=int, default=0, help='N > 0: a synthetic set of N frames instead')
    p.add_argument('--height', type=int, default=180)
    p.add_argument('--width', type=int, default=240)
    p.add_argument('--images', type=int, default=500, help='frames sampled (a seeded permutation of the set)')
    p.add_argument('--per_image', type=int, default=100)
    p.add_argument('--iters', type=int, default=100)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--images_per_pass', type=int, default=24)
    p.add_argument('--dtype', default='f32', choices=['f32', 'bf16'], help='compute type of the backbone')
    return p


def run(flags):
    """What the script does with its parsed flags -> (the model with the seeded head, the record)."""
    from .. import checkpoint
    from ..train import dataset
    from . import nets
    if (flags.synthetic > 0) == bool(flags.csv_root):
        raise SystemExit('one image source: --csv_root/--set/--img_root or --synthetic N')
    dev = torch.device('cuda', torch.cuda.current_device())
    cdt = torch.bfloat16 if flags.dtype == 'bf16' else torch.float32
    model = nets.VGG16NetVLAD(compute_dtype=cdt).to(dev)
    step, missing = load_without_head(model, flags.checkpoint)
    if flags.synthetic > 0:
        image_set = dataset.SyntheticImageSet(flags.synthetic, flags.height, flags.width, seed=flags.seed)
    else:
        image_set = dataset.CsvImageSet(os.path.join(flags.csv_root, flags.set + '.csv'), flags.img_root)
    indices = np.random.RandomState(flags.seed).permutation(len(image_set))[:flags.images]
    rec = init_head(model, image_set, indices, flags.images_per_pass, flags.per_image, flags.iters, flags.seed)
    rec['replaced_checkpoint_head'] = not missing
    checkpoint.save(model, flags.out, global_step=step)
    return model, rec


def main(argv=None):
    _, rec = run(make_parser().parse_args(argv))
    print(rec)
    return rec


if __name__ == '__main__':
    main()

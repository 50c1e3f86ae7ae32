#!/usr/bin/env python
"""Executes residual_det_loss, residual_trace_loss, swrd_loss, ntuplet_evmm_loss,
ntuplet_trace_loss, neg_eigenvalue_loss and ms_sum of the reference's own ``model/losses.py``
(:188-194, 310-370, 613-624) — the file as it lies under /root/reference, nothing of it is
copied — and freezes what they return in tests/golden/golden_ref_eigen_v1.json.
BUILD CONTAINER ONLY: needs /root/reference.

    python tests/tools/ref_exec/make_golden_ref_eigen.py

The losses run on tests/tools/ref_exec/tf_shim.py at FLOAT64 (inputs: the float32 values of
tests/spectral_data.py, widened).  tf_shim refuses ``tf.linalg.svd``, ``tf.slice``,
``tf.linalg.eigh`` and ``tf.linalg.trace`` and has no ``tf.reduce_prod``; this file — not the
shim — supplies NumPy stand-ins: ``np.linalg.svd(x, compute_uv=False)`` (descending, like
TensorFlow's), plain slicing with ``size = -1`` meaning "to the end", ``np.prod``,
``np.linalg.eigh`` (ascending, like TensorFlow's) and ``np.trace`` over the last two axes.  Two
more, because the run is at float64 where the reference's graph is float32: ``tf.zeros`` with the
shim's default dtype replaced by float64 (the hinge's ``tf.zeros([batch])`` meets float64 terms),
and ``tf.negative`` (absent from the shim).  The stand-ins record what they return — singular
values, eigenvalues, traces — from which the per-tuple terms beside each loss are taken and on
which the well-posedness conditions of tests/eigen_data.py are asserted.  ms_sum's ``embeddings``
stay float32 (its ms_loss casts to float32 itself); its anchor / positives / negatives are float64.

Hinge cases: on these inputs ``lambda_min(pos) - lambda_max(neg)`` is far below the reference's
margin of 0.1 and the loss identically 0, so the margin of a hinge case is
``eigen_data.hinge_margin`` of its own raw arguments (one tuple active, one inactive);
ntuplet_trace runs on rows scaled by ``eigen_data.scale_rows(z, seed)``.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_trainer import ROOT  # noqa: E402
import tf_shim  # noqa: E402
from make_golden_ref import load_reference, trainer_ms_labels  # noqa: E402
from tests import eigen_data as ED  # noqa: E402
from tests import spectral_data as D  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'golden_ref_eigen_v1.json')
SVD, SLICES, EIGH, TRACES = [], [], [], []
f64 = np.float64


def _arr(x):
    return tf_shim._t(x).view(np.ndarray)


def _svd(tensor, full_matrices=False, compute_uv=True, name=None):
    assert not compute_uv
    tf_shim._count('linalg.svd')
    s = np.linalg.svd(_arr(tensor), compute_uv=False)
    SVD.append(np.array(s, dtype=f64))
    return tf_shim._t(s)


def _slice(input_, begin, size, name=None):
    tf_shim._count('slice')
    idx = tuple(slice(int(b), None if int(s) == -1 else int(b) + int(s)) for b, s in zip(begin, size))
    out = _arr(input_)[idx]
    SLICES.append(np.array(out, dtype=f64))
    return tf_shim._t(out)


def _eigh(tensor, name=None):
    tf_shim._count('linalg.eigh')
    e, v = np.linalg.eigh(_arr(tensor))
    EIGH.append(np.array(e, dtype=f64))
    return tf_shim._t(e), tf_shim._t(v)


def _trace(x, name=None):
    tf_shim._count('linalg.trace')
    out = np.trace(_arr(x), axis1=-2, axis2=-1)
    TRACES.append(np.array(out, dtype=f64))
    return tf_shim._t(out)


def _zeros(shape, dtype=f64, name=None):
    tf_shim._count('zeros')
    return tf_shim._t(np.zeros([int(d) for d in shape], dtype=dtype))


def _negative(x, name=None):
    tf_shim._count('negative')
    return tf_shim._t(np.asarray(np.negative(_arr(x))))      # (an array: a NumPy scalar would turn float32)


def install_stand_ins():
    tf_shim.linalg.svd = _svd
    tf_shim.linalg.eigh = _eigh
    tf_shim.linalg.trace = _trace
    tf_shim.slice = _slice
    tf_shim.reduce_prod = tf_shim._reduce('reduce_prod', np.prod)
    tf_shim.zeros = _zeros
    tf_shim.negative = _negative


CASES = [   # (T, P, N, E, dimensions, seed)
    (2, 4, 4, 64, 3, 11),
    (3, 5, 7, 200, 4, 12),
    (2, 12, 12, 512, 10, 13),
]
MARGIN = 0.1


def run(R, kind, shape):
    t, p, n, e, k, seed = shape
    z, pw, nw = D.tuples(t, p, n, e, seed)
    if kind == 'ntuplet_trace':
        z = ED.scale_rows(z, seed)
    z = z.astype(f64)
    a, pos, neg = (tf_shim._t(x) for x in (z[:, :1], z[:, 1:1 + p], z[:, 1 + p:]))
    for rec in (SVD, SLICES, EIGH, TRACES):
        del rec[:]
    margin = MARGIN

    def call(m):
        for rec in (SVD, SLICES, EIGH, TRACES):
            del rec[:]
        m = np.array(m, dtype=f64)               # a float64 tensor: a Python float would be float32
        if kind in ('residual_det', 'residual_trace'):
            return getattr(R, kind + '_loss')(a, pos, neg, m, dimensions=k)
        if kind == 'swrd':
            return R.swrd_loss(a, pos, neg, tf_shim._t(pw[:, :p].astype(f64)[:, :, None]),
                               tf_shim._t(nw[:, p:].astype(f64)[:, :, None]), m, dimensions=k)
        if kind in ED.HINGE:
            return getattr(R, kind + '_loss')(a, pos, neg, m)
        if kind == 'neg_eigenvalue':
            return R.neg_eigenvalue_loss(a, neg)
        labels = tf_shim.constant(trainer_ms_labels(t, p, n), dtype=f64)
        # ms_loss casts its masks to float32 (model/losses.py:88-92): its embeddings stay float32, as in
        # make_golden_ref.py; the residual_det part of the sum runs at float64 like the cases above
        emb = tf_shim._t(z.reshape(t * (1 + p + n), e).astype(np.float32))
        return R.ms_sum(a, pos, neg, m, labels, emb, dimensions=k)

    val = call(margin)
    if kind in ED.HINGE:
        # (the reference evaluates the negative side first)
        raw = (EIGH[1][:, 0] - EIGH[0][:, -1]) if kind == 'ntuplet_evmm' else TRACES[1] - TRACES[0]
        margin = ED.hinge_margin(raw)
        val = call(margin)
        args = margin + raw
        floor = 1e-5 if kind == 'ntuplet_evmm' else 1e-3
        assert (args > 0).any() and (args < 0).any() and np.abs(args).min() >= floor, args
    assert np.asarray(val).dtype == f64 and np.asarray(val).shape == ()

    if kind in ED.RESIDUAL + ('ms_sum',):
        assert len(SVD) == 2 and len(SLICES) == 2
        ED.assert_well_posed('residual_det', (SVD[0], SVD[1]), k)
        red = np.sum if kind == 'residual_trace' else np.prod
        terms = np.stack([red(SLICES[0], 1), red(SLICES[1], 1)], 1)
    elif kind == 'ntuplet_evmm':
        ED.assert_well_posed(kind, (EIGH[1], EIGH[0]), k)
        terms = np.stack([EIGH[1][:, 0], EIGH[0][:, -1]], 1)
    elif kind == 'ntuplet_trace':
        terms = np.stack([TRACES[1], TRACES[0]], 1)
    else:
        ED.assert_well_posed(kind, (None, EIGH[0]), k)
        terms = np.stack([np.zeros(t), EIGH[0][:, 0]], 1)
    print('%-15s T%d P%d N%d E%d k%d margin %.9g loss %.12g' % (kind, t, p, n, e, k, margin, float(val)))
    return {'kind': kind, 't': t, 'p': p, 'n': n, 'e': e, 'dimensions': k, 'seed': seed,
            'margin': margin, 'loss': float(val), 'terms': terms.tolist()}


def main():
    install_stand_ins()
    R = load_reference()
    losses = [run(R, kind, shape) for kind in ED.KINDS + ('ms_sum',) for shape in CASES]
    meta = {'made_by': 'tests/tools/ref_exec/make_golden_ref_eigen.py',
            'what': "residual_det_loss, residual_trace_loss, swrd_loss, ntuplet_evmm_loss, ntuplet_trace_loss, "
                    "neg_eigenvalue_loss and ms_sum of /root/reference/model/losses.py at float64 on "
                    "tests/tools/ref_exec/tf_shim.py with NumPy stand-ins for tf.linalg.svd, tf.slice, "
                    "tf.reduce_prod, tf.linalg.eigh, tf.linalg.trace, tf.negative and a float64 tf.zeros "
                    "(inputs: tests/spectral_data.tuples; swrd: pos_w[:, :P], neg_w[:, P:]; ntuplet_trace: "
                    "tests/eigen_data.scale_rows(z, seed); hinge margins: tests/eigen_data.hinge_margin; "
                    "ms_sum: the trainer's labels, embeddings = z as [T(1+P+N), E]); terms = "
                    "[term_pos, term_neg] per tuple",
            'numpy': np.__version__}
    with open(OUT, 'w') as f:
        json.dump({'meta': meta, 'losses': losses}, f, indent=1)
    print('wrote %s' % OUT)


if __name__ == '__main__':
    main()
